"""Times of the dataset fingerprint (csrc/fingerprint.hip, dg_tta_amd/planning/fingerprint.py) on one 256^3 and one 512^3
body-like case (a CT-like ellipsoid in a zero volume, uint8 labels > 0 in an inner ellipsoid):
  * the per-case cost of the three sweeps, each as the driver launches it (sweep 1: first moments + 11-bit histogram; sweep 2:
    centred second moment + 11-bit histogram under the surviving prefixes; sweep 3: 10-bit histogram under the surviving
    prefixes) - device events, warmed up, median, with the rate over the bytes read (4 B image + 1 B label per voxel);
  * the numpy path on the same host: np.percentile (q = 0.5, 50, 99.5), mean and std of the pooled foreground values in float64,
    one run, with the time to pool them (x[seg > 0]);
  * the whole fingerprint of a small synthetic dataset written as .nii.gz (extract_fingerprint: reading, crop, three sweeps) -
    wall clock, everything resident and nothing resident - next to the time reading the files alone takes.

usage: python profiles/tools/fingerprintbench.py [--no-host] [sizes ...]      (default: 256 512)"""
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dg_tta_amd import ops                                                  # noqa: E402
from dg_tta_amd.planning import fingerprint as fp                           # noqa: E402
from dg_tta_amd.tta.nifti_io import write_nifti                             # noqa: E402

DEV = "cuda:0"
REPS, WARMUP = 9, 2
DATASET_CASES, DATASET_SIZE = 6, 160


def body(s, seed=7):
    """(image float32 [s, s, s], labels uint8 [s, s, s]) on the device."""
    ax = (torch.arange(s, dtype=torch.float32, device=DEV) + 0.5) / s - 0.5
    r = (ax[:, None, None] / 0.45) ** 2 + (ax[None, :, None] / 0.40) ** 2 + (ax[None, None, :] / 0.35) ** 2
    g = torch.Generator(device=DEV).manual_seed(seed)
    img = torch.round(torch.randn(s, s, s, device=DEV, generator=g) * 150.0 + 40.0)          # integer-valued, piled up like CT
    img = torch.where(r <= 1.0, torch.where(img == 0, torch.ones_like(img), img), torch.zeros_like(img))
    seg = ((r <= 0.6) * (1 + (torch.rand(s, s, s, device=DEV, generator=g) * 100).to(torch.uint8) % 100)).to(torch.uint8)
    return img.contiguous(), seg.contiguous()


def median_ms(fn):
    times = []
    for rep in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if rep >= WARMUP:
            times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def sweeps(img, seg):
    """Median time of each sweep over the case, with the prefixes the selection really asks for."""
    v = img.numel()
    state = ops.fingerprint_state(DEV)
    counters = ops.fingerprint_counters(DEV, 1)
    ops.fingerprint_sweep(img, seg, counters, moment=1, state=state)
    st = ops.fingerprint_read_state(state)
    mean = st["sum"] / st["count"]
    select = fp.RadixSelect([r for lo, hi, _ in fp.quantile_ranks(st["count"]) for r in (lo, hi)])
    out, bits = [], 0
    for sweep, digit in enumerate(fp.DIGITS):
        n = len(select.prefixes)
        ws = torch.empty(ops.fingerprint_ws_bytes(v, n), dtype=torch.uint8, device=DEV)
        scratch_counters, scratch_state = ops.fingerprint_counters(DEV, n), ops.fingerprint_state(DEV)
        moment = sweep + 1 if sweep < 2 else 0
        prefixes = select.prefixes if bits else None

        def run(c=scratch_counters):
            ops.fingerprint_sweep(img, seg, c, prefix_bits=bits, digit_bits=digit, prefixes=prefixes, moment=moment, state=scratch_state,
                                  mean=mean, ws=ws)
        out.append((median_ms(run), n))
        counters = ops.fingerprint_counters(DEV, n)
        run(counters)
        select.advance(counters.cpu().numpy())
        bits += digit
    return out, st["count"], {r: fp.key_to_float(k) for r, k in select.keys().items()}


def host_seconds(img, seg):
    x, s = img.cpu().numpy(), seg.cpu().numpy()
    t0 = time.perf_counter()
    pooled = x[s > 0].astype(np.float64)
    t1 = time.perf_counter()
    pct = np.percentile(pooled, fp.QUANTILES)
    t2 = time.perf_counter()
    mean, std = pooled.mean(), pooled.std()
    t3 = time.perf_counter()
    return t1 - t0, t2 - t1, t3 - t2, pct, mean, std


def dataset_seconds():
    with tempfile.TemporaryDirectory() as tmp:
        raw = Path(tmp) / "Dataset900_Bench"
        nbytes = 0
        for i in range(DATASET_CASES):
            img, seg = body(DATASET_SIZE, seed=100 + i)
            write_nifti(raw / "imagesTr" / f"case{i}_0000.nii.gz", img.cpu().numpy(), spacing=(1.5, 1.5, 1.5))
            write_nifti(raw / "labelsTr" / f"case{i}.nii.gz", seg.cpu().numpy(), spacing=(1.5, 1.5, 1.5))
            nbytes += img.numel() * 5
        dataset_json = {"labels": {"background": 0, "body": 1}, "file_ending": ".nii.gz", "channel_names": {"0": "CT"},
                        "numTraining": DATASET_CASES}
        listing = fp.training_cases(raw, dataset_json)
        t0 = time.perf_counter()
        for _, images, label in listing:
            fp._read_case(images, label)
        t_read = time.perf_counter() - t0
        fp.extract_fingerprint(raw, dataset_json, device=DEV)                   # warms the allocator and the file cache up
        times = {}
        for name, cache in (("everything resident", 2 ** 34), ("nothing resident", 0)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = fp.extract_fingerprint(raw, dataset_json, device=DEV, cache_bytes=cache)
            torch.cuda.synchronize()
            times[name] = time.perf_counter() - t0
        return t_read, times, nbytes, result


def main():
    host_wanted = "--no-host" not in sys.argv[1:]
    sizes = [int(v) for v in sys.argv[1:] if v != "--no-host"] or [256, 512]
    print(f"device {torch.cuda.get_device_name(0)}", flush=True)
    for s in sizes:
        img, seg = body(s)
        per_sweep, count, order = sweeps(img, seg)
        gb = img.numel() * 5 / 1e9
        line = ", ".join(f"sweep {k + 1} {ms:.3f} ms ({gb / ms * 1e3:.0f} GB/s, {n} prefix{'es' if n > 1 else ''})"
                         for k, (ms, n) in enumerate(per_sweep))
        print(f"{s}^3 body, {count} foreground voxels of {img.numel()}: {line}; three sweeps {sum(ms for ms, _ in per_sweep):.3f} ms",
              flush=True)
        if host_wanted:
            t_pool, t_pct, t_mom, pct, mean, std = host_seconds(img, seg)
            ranks = fp.quantile_ranks(count)
            mine = [order[lo] + (order[hi] - order[lo]) * frac for lo, hi, frac in ranks]
            assert np.allclose(mine, pct, rtol=1e-12, atol=0), (mine, pct)
            print(f"{s}^3 body: host pooling x[seg > 0] {t_pool:.2f} s, np.percentile {t_pct:.2f} s, mean and std {t_mom:.2f} s "
                  f"(percentiles {pct.tolist()}, equal to the device's)", flush=True)
        del img, seg
    t_read, times, nbytes, result = dataset_seconds()
    print(f"dataset of {DATASET_CASES} cases of {DATASET_SIZE}^3 (.nii.gz, {nbytes / 1e6:.0f} MB of voxels): reading and decompressing the files "
          f"alone {t_read:.2f} s; extract_fingerprint {times['everything resident']:.2f} s with everything resident, "
          f"{times['nothing resident']:.2f} s with nothing resident (every case read three times)", flush=True)
    print(f"its intensity block: {result['foreground_intensity_properties_per_channel']['0']}", flush=True)


if __name__ == "__main__":
    main()
