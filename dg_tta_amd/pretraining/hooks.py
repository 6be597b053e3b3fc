"""What the DG trainers' `build_network_architecture` does around the network (reference:
dg_tta/pretraining/nnUNetTrainer_GIN_MIND.py:38-59, nnUNetTrainer_GIN.py:38-58, nnUNetTrainer_MIND.py:37-56): the input
channel count of the descriptor (12 for MIND), internal augmentation switched on, and the forward pre-hooks registered
in the reference's order (gin_hook first, then mind_hook).  The hooks run the HIP kernels (csrc/gin.hip, csrc/mind3d.hip)
for any batch size, GIN with one random kernel chain per batch item (groups = nb, gin.py:168-230)."""
from ..gin import gin_hook  # noqa: F401  (re-exported: the hooks this module registers)
from ..mind import mind_hook  # noqa: F401
from ..tta.nnunet_utils import trainer_hooks, trainer_mirror_axes  # noqa: F401
from ..unet import PLANS_3D_FULLRES, HipPlainConvUNet
from ..utils import enable_internal_augmentation


def trainer_spec(trainer_name):
    """(network input channels, [pre-hooks]) of a DG trainer name (with or without the _MultiRes suffix), or of the stock
    nnUNetTrainer: (1, [])."""
    return trainer_hooks(trainer_name)


def register_dg_hooks(network, trainer_name="nnUNetTrainer_GIN_MIND"):
    """enable_internal_augmentation() + register_forward_pre_hook(gin_hook / mind_hook), as the trainers do.  A trainer
    without hooks (the stock nnUNetTrainer) has no internal augmentation to switch on."""
    _, hooks = trainer_spec(trainer_name)
    if hooks:
        enable_internal_augmentation()
    return [network.register_forward_pre_hook(h) for h in hooks]


def build_network_architecture(cfg=None, trainer_name="nnUNetTrainer_GIN_MIND", act_dtype=None, num_classes=None):
    """The network a DG trainer trains: PlainConvUNet topology from the plans (default: the 3d_fullres plans of the
    reference's model), `num_input_channels` overridden by the trainer, hooks registered."""
    import torch
    cfg = dict(PLANS_3D_FULLRES if cfg is None else cfg)
    cfg["in_channels"], _ = trainer_spec(trainer_name)
    if num_classes is not None:
        cfg["num_classes"] = num_classes
    net = HipPlainConvUNet(cfg, act_dtype=torch.float32 if act_dtype is None else act_dtype)
    register_dg_hooks(net, trainer_name)
    return net
