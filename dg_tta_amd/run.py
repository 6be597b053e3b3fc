"""`dgtta` command line — same sub-commands, positional arguments and option names as the reference's dg_tta/run.py
(prepare_tta :71-118, run_tta :120-209).  `pretrain` takes the arguments of `nnUNetv2_train`, which the reference dispatches
into, and trains on this engine (pretraining/trainer.py); `inject_trainers` patches an installed nnunetv2 and has nothing
to do here.  `plan` stands for the planning half of `nnUNetv2_plan_and_preprocess`: the dataset fingerprint (on the GPU) and nnU-Net
2.2.1's ExperimentPlanner (planning/), so that `pretrain` can start from a raw dataset.  `predict` takes the arguments of
`nnUNetv2_predict` and applies a trained model folder to a folder of images without adaptation (predict.py).  Extra, optional: `run_tta --gpus N` fans out one process per GPU
(sample-sharded, no collectives), `--dtype {fp32,bf16,fp16}` (default fp32 = the reference's precision).
"""
import argparse
import json
import os
import re
import subprocess
import sys
from datetime import datetime
from pathlib import Path

import torch

from .utils import check_dga_root_is_set
from .tta.torch_utils import generate_label_mapping
from .tta.config_log_utils import (check_dataset_pretrain_config, get_tta_folders, load_current_modifier_functions,
                                   prepare_tta as _prepare_tta)

DEFAULT_DTYPE = "fp32"      # activation storage of `run_tta`: the reference's precision (dg_tta/tta/tta.py:560 never autocasts); it is
                            # the setting that keeps north_star's bit-exact label maps (tests/test_gpu_tta.py::test_tta_unit_golden)
FAST_DTYPE = "fp16"         # opt-in 16-bit storage (`--dtype fp16|bf16`).  fp16 (guarded loss scale; BASELINE config 5's mixed precision) is
                            # the headline dtype of bench.py since round 6: the 16-bit type that meets the stated parity tolerances
                            # against the oracle (tests/test_gpu_referee.py) at the same rate as bf16 (BASELINE config 2's name)

_ADJ = ("brisk", "calm", "eager", "fuzzy", "keen", "lucid", "mellow", "nimble", "quiet", "rapid", "solid", "vivid")
_NOUN = ("atlas", "beacon", "cortex", "delta", "ember", "fjord", "gamma", "harbor", "isthmus", "kernel", "lattice", "voxel")


def _random_name():
    """`randomname.get_name()` stand-in (package not installable offline): adjective-noun."""
    import random
    r = random.SystemRandom()
    return f"{r.choice(_ADJ)}-{r.choice(_NOUN)}"


def _add_common(parser):
    parser.add_argument("pretrained_dataset_id", help="Task ID for pretrained model. Can be numeric or one of "
                        "['TS104_GIN', 'TS104_MIND', 'TS104_GIN_MIND']")
    parser.add_argument("tta_dataset_id", help="Task ID for TTA")
    parser.add_argument("--pretrainer", help="Trainer to use for pretraining", default=None)
    parser.add_argument("--pretrainer_config", help="Fold ID of nnUNet model to use for pretraining", default="3d_fullres")
    parser.add_argument("--pretrainer_fold", help="Fold ID of nnUNet model to use for pretraining", default="0")


def _wait_children(procs, poll_s=0.5):
    """Waits for the per-GPU children; when one fails the others are stopped (they would otherwise sit in the filesystem
    barrier waiting for the dead rank's files).  Returns the list of return codes."""
    import time
    while True:
        rcs = [p.poll() for p in procs]
        if all(rc is not None for rc in rcs):
            return rcs
        if any(rc is not None and rc != 0 for rc in rcs):
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            return [p.wait() for p in procs]
        time.sleep(poll_s)


class DGTTAProgram:
    def __init__(self, argv=None):
        self.argv = list(sys.argv if argv is None else argv)
        parser = argparse.ArgumentParser(description="DG-TTA for nnUNetv2 (MI355X engine)", usage="""dgtta <command> [<args>]

        Commands are:
        plan            Fingerprint the source dataset and plan the experiment (writes nnUNetPlans.json)
        pretrain        Pre-train on the source dataset (GIN / MIND trainers)
        prepare_tta     Prepare test-time adaptation
        run_tta         Run test-time adaptation
        predict         Predict a folder of images with a trained model (fold ensemble, no adaptation)
        """)
        parser.add_argument("command", help="Subcommand to run")
        args = parser.parse_args(self.argv[1:2])
        if args.command.startswith("_") or not hasattr(self, args.command):
            print("Unrecognized command")
            parser.print_help()
            raise SystemExit(1)
        getattr(self, args.command)()

    def inject_trainers(self):
        raise SystemExit("inject_trainers patches an installed nnunetv2 so that nnUNetv2_train finds the DG trainers; "
                         "nothing is injected here: `dgtta pretrain` trains on this engine and no longer needs it.")

    def plan(self):
        parser = argparse.ArgumentParser(description="Fingerprint the raw source dataset on the GPU and plan the experiment as "
                                         "nnU-Net 2.2.1's ExperimentPlanner does (nnUNetv2_plan_and_preprocess without the eager "
                                         "preprocessing)", usage="dgtta plan [-h]")
        parser.add_argument("dataset_id", help="Dataset name or numeric id of the source dataset in nnUNet_raw")
        parser.add_argument("--device", help="Device of the fingerprint sweeps; 'cpu' runs them in numpy", default="cuda")
        parser.add_argument("--cache_gib", type=float, default=64.0,
                            help="device memory (GiB) the cropped cases may occupy between the sweeps; the rest is read from disk "
                                 "again.  The result does not depend on it")
        parser.add_argument("--overwrite", action="store_true", help="replace an existing nnUNetPlans.json")
        args = parser.parse_args(self.argv[2:])
        from .planning.fingerprint import extract_fingerprint
        from .planning.planner import channel_schemes, plan_experiment
        from .tta.config_log_utils import maybe_convert_to_dataset_name, nnunet_path
        dataset_name = maybe_convert_to_dataset_name(args.dataset_id)
        raw = Path(nnunet_path("nnUNet_raw")) / dataset_name
        pre = Path(nnunet_path("nnUNet_preprocessed")) / dataset_name
        if not (raw / "dataset.json").is_file():
            raise SystemExit(f"plan: {raw / 'dataset.json'} not found")
        plans_file = pre / "nnUNetPlans.json"
        if plans_file.is_file() and not args.overwrite:
            raise SystemExit(f"plan: {plans_file} exists; pass --overwrite to replace it")
        with open(raw / "dataset.json") as f:
            dataset_json = json.load(f)
        try:
            channel_schemes(dataset_json)               # a dataset.json the planner refuses costs no sweep and leaves no file
        except ValueError as e:
            raise SystemExit(f"plan: {raw / 'dataset.json'}: {e}") from e
        fingerprint = extract_fingerprint(raw, dataset_json, device=torch.device(args.device), cache_bytes=int(args.cache_gib * 2 ** 30),
                                          output_file=pre / "dataset_fingerprint.json")
        plans = plan_experiment(fingerprint, dataset_json, dataset_name=dataset_name)
        for name, content in (("nnUNetPlans.json", plans), ("dataset.json", dataset_json)):
            with open(pre / name, "w") as f:
                json.dump(content, f, indent=4)
        for name, conf in plans["configurations"].items():
            if "inherits_from" in conf:
                print(f"plan: {name}: inherits from {conf['inherits_from']}, previous stage {conf['previous_stage']}")
            else:
                print(f"plan: {name}: spacing {conf['spacing']}, median shape {conf['median_image_size_in_voxels']}, patch "
                      f"{conf['patch_size']}, batch {conf['batch_size']}, {len(conf['pool_op_kernel_sizes'])} stages, "
                      f"{conf['normalization_schemes']}")
        print(f"plan: wrote {plans_file}.  Not planned: `2d` (no 2-D kernels here), ResEnc planners, the `architecture` schema of "
              f"nnU-Net >= 2.4.  `3d_lowres` and the cascade are written when nnU-Net would plan them; training the cascade is not "
              f"built.  Nothing is preprocessed now: `dgtta pretrain` preprocesses each case on first use.  The intensity "
              f"statistics are exact over all foreground voxels (nnU-Net samples 10 000 per case).")

    @staticmethod
    def _pretrain_parser(trainers=None):
        """trainers: the names `-tr` takes.  The bare parser keeps the six DG trainers it always took (callers and tests that
        build it themselves see no change); the `pretrain` command asks for TRAINERS, which adds the stock nnUNetTrainer."""
        from .pretraining.trainer import DG_TRAINERS
        trainers = DG_TRAINERS if trainers is None else tuple(trainers)
        parser = argparse.ArgumentParser(description="Pre-train a DG trainer's network on the source dataset (positional "
                                         "arguments, -tr and --c as in nnUNetv2_train)", usage="dgtta pretrain [-h]")
        parser.add_argument("dataset_id", help="Dataset name or numeric id of the source dataset")
        parser.add_argument("configuration", help="Configuration of nnUNetPlans.json, e.g. 3d_fullres")
        parser.add_argument("fold", help="Fold of the 5-fold split, 0..4, or 'all'")
        parser.add_argument("-tr", dest="trainer", required=True, choices=trainers,
                            help="DG trainer, or the stock nnUNetTrainer (the baseline: no hooks, mirroring)")
        parser.add_argument("--num_epochs", type=int, default=1000)
        parser.add_argument("--iterations_per_epoch", type=int, default=250)
        parser.add_argument("--val_iterations", type=int, default=50)
        parser.add_argument("--device", help="Device to be used", default="cuda")
        parser.add_argument("--dtype", choices=["fp32", "fp16", "bf16"], default=DEFAULT_DTYPE, help="activation storage")
        parser.add_argument("--c", dest="continue_training", action="store_true",
                            help="continue from fold_<k>/checkpoint_latest.pth")
        parser.add_argument("--seed", type=int, default=None, help="seeds the initialisation and every random draw")
        parser.add_argument("--augmentation", choices=["reduced", "spatial", "full"], default="reduced",
                            help="spatial: nnU-Net's rotation / scaling on the training batches; full: that plus its noise / blur / "
                                 "brightness / contrast / low-resolution / gamma chain")
        parser.add_argument("--dice", choices=["sample", "plans"], default="sample",
                            help="sample: the Dice term of the loss per sample, whatever the plans say; plans: pooled over the batch "
                                 "when the configuration's batch_dice is true, as nnU-Net trains it")
        parser.add_argument("--validate", action="store_true",
                            help="after training, predict every validation case of the fold with checkpoint_final.pth and write "
                                 "fold_<k>/validation/ (label maps and summary.json, in the preprocessed geometry)")
        parser.add_argument("--val", dest="validation_only", action="store_true",
                            help="do not train: run that validation on the fold's existing checkpoint_final.pth")
        return parser

    def pretrain(self):
        from .pretraining.trainer import TRAINERS
        args = self._pretrain_parser(TRAINERS).parse_args(self.argv[2:])
        if args.fold != "all" and not args.fold.isnumeric():
            raise SystemExit(f"pretrain: fold {args.fold!r} is neither a number nor 'all'")
        from .pretraining.trainer import FULL_AUGMENTATION_NOTE, REDUCED_AUGMENTATION_NOTE, SPATIAL_AUGMENTATION_NOTE, train_fold
        act_dtype = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
        if args.validation_only:
            from .pretraining.trainer import validate_fold
            summary = validate_fold(args.dataset_id, args.configuration, args.fold, args.trainer, device=torch.device(args.device),
                                    act_dtype=act_dtype)
            print(f"pretrain: validated {len(summary['metric_per_case'])} cases, foreground mean Dice "
                  f"{summary['foreground_mean']['Dice']:.4f}")
            return
        print({"spatial": SPATIAL_AUGMENTATION_NOTE, "full": FULL_AUGMENTATION_NOTE}.get(args.augmentation, REDUCED_AUGMENTATION_NOTE))
        from .pretraining.hooks import trainer_mirror_axes
        axes = trainer_mirror_axes(args.trainer)
        if axes is not None:
            print(f"pretrain: {args.trainer} - no GIN / MIND hooks; nnU-Net's mirroring IS applied to the training batches along axes "
                  f"{list(axes)} (each with probability 0.5, after the other transforms) and the checkpoint allows the same axes at "
                  f"inference (inference_allowed_mirroring_axes).")
        final = train_fold(args.dataset_id, args.configuration, args.fold, args.trainer, num_epochs=args.num_epochs,
                           iterations_per_epoch=args.iterations_per_epoch, val_iterations=args.val_iterations,
                           device=torch.device(args.device), continue_training=args.continue_training, seed=args.seed, augmentation=args.augmentation,
                           act_dtype=act_dtype, dice=args.dice, final_validation=args.validate)
        print(f"pretrain: wrote {final}")

    @staticmethod
    def _predict_parser():
        """nnUNetv2_predict's arguments and defaults (nnunetv2 2.2.1, from memory: unpinned).  Not accepted: -npp, -nps,
        -prev_stage_predictions, -num_parts / -part_id (one process, one GPU) and the postprocessing_* plan keys."""
        parser = argparse.ArgumentParser(description="Predict a folder of images with the ensemble of a trained model's folds "
                                         "(arguments as in nnUNetv2_predict; no test-time adaptation, no post-processing)",
                                         usage="dgtta predict [-h]")
        parser.add_argument("-i", dest="input_folder", required=True,
                            help="folder of images: <case>_0000.<ext> (NIfTI / NRRD / MetaImage), or preprocessed .npy / .npz arrays")
        parser.add_argument("-o", dest="output_folder", required=True, help="folder the label maps are written to")
        parser.add_argument("-d", dest="dataset_id", required=True, help="Dataset name or numeric id the model was trained on")
        parser.add_argument("-c", dest="configuration", required=True, help="Configuration of the plans, e.g. 3d_fullres")
        parser.add_argument("-tr", dest="trainer", default="nnUNetTrainer", help="trainer of the model folder")
        parser.add_argument("-p", dest="plans", default="nnUNetPlans", help="plans identifier of the model folder")
        parser.add_argument("-f", dest="folds", nargs="+", default=["0", "1", "2", "3", "4"],
                            help="folds whose checkpoints form the ensemble: numbers, or 'all'")
        parser.add_argument("-chk", dest="checkpoint_name", default="checkpoint_final.pth")
        parser.add_argument("--disable_mirroring", "--disable_tta", dest="disable_mirroring", action="store_true",
                            help="no mirrored passes, whatever the checkpoint allows.  --disable_tta is nnU-Net's name for the same "
                                 "switch: it means mirroring and has nothing to do with DG-TTA")
        parser.add_argument("--save_probabilities", action="store_true",
                            help="also write <case>.npz: softmax probabilities of every class (label models, at most 32 classes) or "
                                 "sigmoid probabilities of every region (region models), float16")
        parser.add_argument("--continue_prediction", action="store_true", help="skip the cases whose output files exist")
        parser.add_argument("--device", help="Device to be used", default="cuda")
        parser.add_argument("--dtype", choices=["fp32", "fp16", "bf16"], default=DEFAULT_DTYPE, help="activation storage")
        return parser

    def predict(self):
        args = self._predict_parser().parse_args(self.argv[2:])
        for k in args.folds:
            if k != "all" and not k.isnumeric():
                raise SystemExit(f"predict: fold {k!r} is neither a number nor 'all'")
        from .predict import model_folder_of, predict_from_model_folder
        folder = model_folder_of(args.dataset_id, args.configuration, args.trainer, args.plans)
        try:
            written = predict_from_model_folder(
                folder, args.input_folder, args.output_folder, folds=[k if k == "all" else int(k) for k in args.folds],
                checkpoint_name=args.checkpoint_name, device=torch.device(args.device),
                act_dtype={"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype],
                use_mirroring=not args.disable_mirroring, save_probabilities=args.save_probabilities,
                continue_prediction=args.continue_prediction)
        except FileNotFoundError as e:
            raise SystemExit(f"predict: {e}") from e
        print(f"predict: wrote {len(written)} label maps to {args.output_folder}")

    def prepare_tta(self):
        parser = argparse.ArgumentParser(description="Prepare DG-TTA", usage="dgtta prepare_tta [-h]")
        _add_common(parser)
        parser.add_argument("--tta_dataset_bucket", help="Can be one of ['imagesTr', 'imagesTs', 'imagesTrAndTs']",
                            default="imagesTs")
        args = parser.parse_args(self.argv[2:])
        ds, trainer, cfg, fold = check_dataset_pretrain_config(args.pretrained_dataset_id, args.pretrainer,
                                                               args.pretrainer_config, args.pretrainer_fold)
        _prepare_tta(ds, int(args.tta_dataset_id), pretrainer=trainer, pretrainer_config=cfg, pretrainer_fold=fold,
                     tta_dataset_bucket=args.tta_dataset_bucket)

    def run_tta(self):
        parser = argparse.ArgumentParser(description="Run DG-TTA")
        _add_common(parser)
        parser.add_argument("--device", help="Device to be used", default="cuda")
        parser.add_argument("--gpus", type=int, default=1, help="one TTA process per GPU, samples sharded round-robin")
        parser.add_argument("--dtype", choices=["fp32", "bf16", "fp16"], default=DEFAULT_DTYPE,
                            help="activation storage: fp32 (default) = the reference's precision, reproduces its label maps; "
                                 "fp16 / bf16 = opt-in 16-bit storage with fp32 accumulation at ~5.5x the fp32 rate.  Measured on a "
                                 "pre-trained synthetic model against the CPU restatement of the reference's loop "
                                 "(tests/test_gpu_referee.py, profiles/r0*_dice_delta_12_epochs*.json): fp16 (guarded loss scale) "
                                 "stays within 1e-3 of the reference's Dice AND of its per-epoch loss; bf16 holds the Dice on a "
                                 "well-trained model (2e-3 off on a weaker one) but not the loss - prefer fp16; "
                                 "not measured on real TS104 weights (no network here): check on your data")
        parser.add_argument("--run_name", default=None,
                            help="name of the run directory (default: timestamp + random name).  Required, and the same on "
                                 "every rank, when RANK / WORLD_SIZE are set by an external launcher")
        args = parser.parse_args(self.argv[2:])
        ds, trainer, cfg, fold = check_dataset_pretrain_config(args.pretrained_dataset_id, args.pretrainer,
                                                               args.pretrainer_config, args.pretrainer_fold)
        tta_data_dir, plan_dir, results_dir, pre_name, tta_name = get_tta_folders(ds, int(args.tta_dataset_id), trainer,
                                                                                  cfg, fold)
        if (Path(plan_dir) / "tta_plan.json").is_file():      # a region-based model is refused before any directory is made
            from .labels import refuse_region_tta_of_weights
            with open(Path(plan_dir) / "tta_plan.json", "r") as f:
                weights = json.load(f).get("pretrained_weights_filepath")
            if weights:
                refuse_region_tta_of_weights(weights, f"run_tta: {weights}")
        run_name = args.run_name
        if run_name is None and int(os.environ.get("WORLD_SIZE", 1)) > 1:
            # every rank would invent its own timestamp + random name and then wait for the others in a directory of its own
            raise SystemExit("run_tta: WORLD_SIZE > 1 needs --run_name (the same on every rank); `--gpus N` sets it itself")
        if int(os.environ.get("WORLD_SIZE", 1)) > 1:
            from .sharding import launch_id
            if not launch_id():
                # the done / failed markers of two launches into one run directory could not be told apart
                raise SystemExit("run_tta: WORLD_SIZE > 1 under a launcher other than torch.distributed.run needs DGTTA_LAUNCH_ID "
                                 "(any string that is the same on every rank and new for every launch)")
        if run_name is None:
            now_str = datetime.now().strftime("%Y%m%d__%H_%M_%S")
            results_dir.mkdir(exist_ok=True, parents=True)
            numbers = [int(m[0]) for m in (re.search(r"[0-9]+$", str(p)) for p in results_dir.iterdir()) if m]
            run_no = 0 if len(numbers) == 0 else max(numbers) + 1
            run_name = f"{now_str}_{_random_name()}-{run_no}"

        rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
        if args.gpus > 1 and world == 1:
            # fan out: one independent process per GPU, pinned with HIP_VISIBLE_DEVICES, same run directory
            (results_dir / run_name).mkdir(exist_ok=True, parents=True)
            from .sharding import child_devices
            import uuid
            procs, launch = [], uuid.uuid4().hex
            for r, dev_id in enumerate(child_devices(args.gpus)):
                env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(args.gpus), HIP_VISIBLE_DEVICES=dev_id,
                           DGTTA_SUMMARY_BY_PARENT="1", DGTTA_LAUNCH_ID=launch)
                env.pop("CUDA_VISIBLE_DEVICES", None)
                cmd = [sys.executable, "-m", "dg_tta_amd.run"] + self.argv[1:] + ["--run_name", run_name]
                procs.append(subprocess.Popen(cmd, env=env))
            rcs = _wait_children(procs)
            if any(rc != 0 for rc in rcs):       # a child killed by a signal has a NEGATIVE return code
                print(f"run_tta: child return codes {rcs}: not evaluating an incomplete run", file=sys.stderr)
                raise SystemExit(1)
            # every child has exited: all predictions are on disk, the summary cannot race (reference: tta.py:447-470)
            with open(Path(plan_dir) / "tta_plan.json", "r") as f:
                config = json.load(f)
            from .tta.tta import evaluate_run
            evaluate_run(results_dir / run_name, config, load_current_modifier_functions(plan_dir), torch.device(args.device))
            raise SystemExit(0)

        with open(Path(plan_dir) / "tta_plan.json", "r") as f:
            config = json.load(f)
        with open(Path(plan_dir) / f"{pre_name}_label_mapping.json", "r") as f:
            pretrained_label_mapping = json.load(f)
        with open(Path(plan_dir) / f"{tta_name}_label_mapping.json", "r") as f:
            tta_dataset_label_mapping = json.load(f)
        label_mapping = generate_label_mapping(pretrained_label_mapping, tta_dataset_label_mapping)
        modifier_fn_module = load_current_modifier_functions(plan_dir)
        from .tta.tta import tta_main
        (results_dir / run_name).parent.mkdir(exist_ok=True, parents=True)
        tta_main(run_name=run_name, config=config, tta_data_dir=tta_data_dir, save_base_path=results_dir,
                 label_mapping=label_mapping, modifier_fn_module=modifier_fn_module, device=torch.device(args.device),
                 shard=(rank, world),
                 act_dtype={"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype])


def main():
    if len(sys.argv) == 1 or sys.argv[1] in ["--help", "-h"]:
        check_dga_root_is_set(soft_check=True)
    else:
        check_dga_root_is_set()
    DGTTAProgram()


if __name__ == "__main__":
    main()
