"""Dataset fingerprint: what nnU-Net's DatasetFingerprintExtractor writes to dataset_fingerprint.json [3P nnunetv2==2.2.1:
experiment_planning/dataset_fingerprint/fingerprint_extractor.py], restated from its published behaviour - per training case the
shape after the crop to the non-zero box, the spacing and the relative size after cropping, and per image channel the intensity
statistics of the foreground voxels (label > 0) pooled over all cases.

The intensity statistics here are EXACT over all foreground voxels.  nnU-Net draws 10 000 foreground voxels per case and takes
np.percentile / mean / std of the pooled sample: its numbers are a sampled estimate of the same quantities, so the two agree to
sampling error only, and this block is UNPINNED (no nnU-Net output to compare with).  Exact statistics need no random stream
and are three bandwidth-bound sweeps over the cropped cases on the device (csrc/fingerprint.hip):
  sweep 1  count, min, max, sum x (double), non-finite count; histogram of the first 11 bits of the order-preserving key
  sweep 2  sum (x - mean)^2 (double) around the pooled mean; histogram of the next 11 bits under the <= 6 surviving prefixes
  sweep 3  histogram of the last 10 bits
The host reads the counters after each sweep (one small copy per channel and sweep, none per case) and picks the prefixes
that hold the at most six ranks np.percentile(..., method="linear") needs for q = 0.5, 50, 99.5.  Cropped cases stay resident
in device memory while they fit in `cache_bytes`; the others are read from disk again in sweeps 2 and 3.  The sums are added in
case order with a fixed partition inside a case, so the result does not depend on the budget.  device="cpu" runs the same
definitions in numpy float64 on the pooled foreground values (slow; needs them in host memory)."""
import json
import math
from pathlib import Path

import numpy as np
import torch

from ..tta.image_io import read_image
from ..tta.preprocessing import crop_to_nonzero, nonzero_box_gpu

DIGITS = (11, 11, 10)                      # 2048-bin histograms: 8 KB of LDS per prefix (65 536 bins would not fit)
QUANTILES = (0.5, 50.0, 99.5)
DEFAULT_CACHE_BYTES = 64 * 2 ** 30


# ------------------------------------------------------------------------------------------------ order statistics (host side)
def float_key(x):
    """Order-preserving uint32 key of float32 values: sign bit flipped for a clear sign bit, all bits inverted otherwise."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(key):
    key = int(key)
    u = key ^ 0x80000000 if key & 0x80000000 else (~key) & 0xFFFFFFFF
    return float(np.array([u], dtype=np.uint32).view(np.float32)[0])


def quantile_ranks(n, quantiles=QUANTILES):
    """[(lower rank, upper rank, fraction)] of np.percentile(x, q, method="linear") over n values."""
    out = []
    for q in quantiles:
        pos = (q / 100.0) * (n - 1)
        lo = int(math.floor(pos))
        out.append((lo, min(lo + 1, n - 1), pos - lo))
    return out


class RadixSelect:
    """Exact selection of a few ranks from digit histograms.  ranks: 0-based ranks in the sorted values.  After every sweep
    `advance` takes the counters [len(self.prefixes), 2048] of that sweep; `prefixes` are then those of the next sweep and,
    after the last digit, the keys themselves (`keys()`)."""

    def __init__(self, ranks, digits=DIGITS):
        self.digits = tuple(digits)
        self.level = 0
        self.prefix_bits = 0
        self.prefixes = [0]
        self.items = {int(r): (0, int(r)) for r in set(ranks)}       # rank -> (prefix, rank among the keys with that prefix)

    @property
    def done(self):
        return self.level == len(self.digits)

    @property
    def digit_bits(self):
        return self.digits[self.level]

    def advance(self, counters):
        counters = np.asarray(counters).astype(np.uint64)
        bits = self.digit_bits
        for rank, (prefix, residual) in self.items.items():
            row = counters[self.prefixes.index(prefix), :1 << bits]
            cum = np.cumsum(row)
            digit = int(np.searchsorted(cum, residual, side="right"))
            if digit >= len(row):
                raise RuntimeError(f"radix select: rank {rank} is beyond the {int(cum[-1])} values counted under its prefix")
            self.items[rank] = ((prefix << bits) | digit, residual - (int(cum[digit - 1]) if digit else 0))
        self.prefix_bits += bits
        self.level += 1
        self.prefixes = sorted({p for p, _ in self.items.values()})

    def keys(self):
        assert self.done
        return {rank: prefix for rank, (prefix, _) in self.items.items()}


def finish_statistics(count, vmin, vmax, total, sumsq_centred, order):
    """The channel's block of the fingerprint from the exact sums and the order statistics {rank: value}."""
    props = {"max": float(vmax), "mean": total / count, "min": float(vmin), "std": math.sqrt(sumsq_centred / count)}
    for name, (lo, hi, frac) in zip(("percentile_00_5", "median", "percentile_99_5"), quantile_ranks(count)):
        props[name] = order[lo] + (order[hi] - order[lo]) * frac
    return {k: props[k] for k in ("max", "mean", "median", "min", "percentile_00_5", "percentile_99_5", "std")}


# ------------------------------------------------------------------------------------------------ cases
def training_cases(raw_dataset_dir, dataset_json):
    """[(name, [image file per channel], label file)] of imagesTr / labelsTr, sorted by name."""
    raw = Path(raw_dataset_dir)
    ending = dataset_json.get("file_ending", ".nii.gz")
    channels = len(dataset_json.get("channel_names", dataset_json.get("modality", {"0": ""})))
    labels = sorted(p for p in (raw / "labelsTr").iterdir() if p.name.endswith(ending)) if (raw / "labelsTr").is_dir() else []
    if not labels:
        raise FileNotFoundError(f"no *{ending} file in {raw / 'labelsTr'}")
    cases = []
    for lab in labels:
        name = lab.name[:-len(ending)]
        images = [raw / "imagesTr" / f"{name}_{c:04d}{ending}" for c in range(channels)]
        missing = [str(p) for p in images if not p.is_file()]
        if missing:
            raise FileNotFoundError(f"case {name}: {missing} not found")
        cases.append((name, images, lab))
    return cases


def _read_case(images, label):
    data, hdr = [], None
    for f in images:
        arr, hdr = read_image(f)
        data.append(np.asarray(arr, dtype=np.float32))
    seg = read_image(label)[0]
    if any(d.shape != seg.shape for d in data):
        raise ValueError(f"{label}: label map {seg.shape} and image {[d.shape for d in data]} differ in shape")
    return np.stack(data), seg, [float(s) for s in hdr["pixdim"][::-1]]          # (z, y, x), as SimpleITK's GetSpacing()[::-1]


def _label_tensor_dtype(seg):
    """The narrowest of the kernels' label types that holds the label map's values."""
    if seg.dtype == np.uint8:
        return np.uint8
    if seg.dtype in (np.int8, np.int16):
        return np.int16
    if np.issubdtype(seg.dtype, np.integer) and seg.size and int(seg.min()) >= -2 ** 31 and int(seg.max()) < 2 ** 31:
        return np.int32
    if np.issubdtype(seg.dtype, np.floating) and np.array_equal(seg, np.round(seg)) and np.abs(seg).max(initial=0) < 2 ** 31:
        return np.int32
    raise ValueError(f"label map of type {seg.dtype} does not hold 32-bit integer labels")


class _Cases:
    """The cropped cases of a dataset: geometry read once, voxels resident on the device while they fit, else re-read."""

    def __init__(self, cases, device, cache_bytes):
        self.cases, self.device, self.gpu = cases, torch.device(device), torch.device(device).type == "cuda"
        self.left = int(cache_bytes)
        self.boxes, self.resident = [], {}
        self.shapes, self.spacings, self.relative_sizes = [], [], []

    def scan(self):
        """The first pass: reads and crops every case, records its geometry, keeps it if it fits; yields (index, data, seg).
        On a GPU the volume goes up once: the non-zero box is found on the device (nonzero_box_gpu) and the channels are cut
        there.  A case of 2^31 - 1 voxels or more (the hole-filling kernels name components by int32) is cropped on the host."""
        assert not self.boxes, "scan() runs once"
        for index, (name, images, label) in enumerate(self.cases):
            data, seg, spacing = _read_case(images, label)
            full = None
            if self.gpu and data[0].size < 2 ** 31 - 1:
                full = torch.from_numpy(data).to(self.device)
                bbox = nonzero_box_gpu(full)[1]
            else:
                bbox = crop_to_nonzero(data, None)[2]
            shape = [b - a for a, b in bbox]
            self.boxes.append(bbox)
            self.shapes.append(shape)
            self.spacings.append(spacing)
            self.relative_sizes.append(float(np.prod(shape, dtype=np.float64) / np.prod(data.shape[1:], dtype=np.float64)))
            case = self._cut(data if full is None else full, seg, bbox)
            del full
            self._keep(index, case)
            yield (index, *case)

    def again(self):
        """A later pass: resident cases from memory, the others from disk; yields (index, data, seg)."""
        for index in range(len(self.cases)):
            yield (index, *self.load(index))

    def _cut(self, data, seg, bbox):
        """(channels, labels) of the box.  On a GPU every channel is a tensor of its own: an allocation is 16-byte aligned
        whatever the voxel count, so every channel takes the kernels' 16-byte loads (a slice of one [C, ...] tensor would not
        when the count is no multiple of 4)."""
        sl = tuple(slice(a, b) for a, b in bbox)
        seg = np.ascontiguousarray(seg[sl]).astype(_label_tensor_dtype(seg), copy=False)
        if not self.gpu:
            return np.ascontiguousarray(data[(slice(None),) + sl]), seg
        if not isinstance(data, torch.Tensor):
            data = torch.from_numpy(np.ascontiguousarray(data[(slice(None),) + sl])).to(self.device)
            sl = (slice(None),) * 3
        return [data[c][sl].clone(memory_format=torch.contiguous_format) for c in range(data.shape[0])], torch.from_numpy(seg).to(self.device)

    def _keep(self, index, case):
        data, seg = case
        nbytes = sum(d.numel() * 4 for d in data) + seg.numel() * seg.element_size() if self.gpu else 0
        if self.gpu and nbytes <= self.left:            # (the host path pools the foreground values: nothing to keep)
            self.left -= nbytes
            self.resident[index] = case

    def __len__(self):
        return len(self.cases)

    def name(self, index):
        return self.cases[index][0]

    def load(self, index):
        """(channels, seg [z, y, x]) of the cropped case: on a GPU a list of float32 device tensors [z, y, x] and a device tensor,
        on the host a numpy array [C, z, y, x] and a numpy array."""
        if index in self.resident:
            return self.resident[index]
        _, images, label = self.cases[index]
        data, seg, _ = _read_case(images, label)
        return self._cut(data, seg, self.boxes[index])


# ------------------------------------------------------------------------------------------------ intensity statistics
def _nonfinite_error(name, channel):
    return ValueError(f"fingerprint: case {name} has a non-finite (NaN / inf) value in the foreground of channel {channel}")


def _no_foreground_error(channel):
    return ValueError(f"fingerprint: no training case has a foreground voxel (label > 0) in channel {channel}")


class MemoryCases:
    """Cases that are device tensors already: [(name, channels, seg)], channels a float32 tensor [C, ...] or a list of C
    tensors, seg [...] uint8 / int16 / int32."""

    def __init__(self, cases, device):
        self.cases, self.device, self.gpu = list(cases), torch.device(device), True

    def scan(self):
        for index, (_, data, seg) in enumerate(self.cases):
            yield index, data, seg

    again = scan

    def __len__(self):
        return len(self.cases)

    def name(self, index):
        return self.cases[index][0]


def pooled_statistics_gpu(cases, channels):
    """Per channel {count, min, max, sum, sumsq_centred, order: {rank: value}} of the pooled foreground, three sweeps over
    `cases` (a _Cases on a GPU, or MemoryCases)."""
    from .. import ops
    dev = cases.device
    states = [ops.fingerprint_state(dev) for _ in range(channels)]
    selects, means = [None] * channels, [0.0] * channels
    first = {}
    for sweep in range(len(DIGITS)):
        prefix_bits = sum(DIGITS[:sweep])
        counters = [ops.fingerprint_counters(dev, 1 if sweep == 0 else len(selects[c].prefixes)) for c in range(channels)]
        for index, data, seg in (cases.scan() if sweep == 0 else cases.again()):
            for c in range(channels):
                ops.fingerprint_sweep(data[c], seg, counters[c], prefix_bits=prefix_bits, digit_bits=DIGITS[sweep],
                                      prefixes=None if sweep == 0 else selects[c].prefixes, moment=sweep + 1 if sweep < 2 else 0,
                                      state=states[c], mean=means[c], case_index=index)
        for c in range(channels):
            if sweep == 0:
                first[c] = st = ops.fingerprint_read_state(states[c])
                if st["nonfinite"]:
                    raise _nonfinite_error(cases.name(st["first_nonfinite_case"]), c)
                if st["count"] == 0:
                    raise _no_foreground_error(c)
                means[c] = st["sum"] / st["count"]
                selects[c] = RadixSelect([r for lo, hi, _ in quantile_ranks(st["count"]) for r in (lo, hi)])
            selects[c].advance(counters[c].cpu().numpy())
    out = []
    for c in range(channels):
        st = dict(first[c], sumsq_centred=ops.fingerprint_read_state(states[c])["sumsq_centred"])
        st["order"] = {rank: key_to_float(key) for rank, key in selects[c].keys().items()}
        out.append(st)
    return out


def intensity_statistics_gpu(cases, channels):
    """Per channel the block of the fingerprint, from pooled_statistics_gpu."""
    return {str(c): finish_statistics(st["count"], st["min"], st["max"], st["sum"], st["sumsq_centred"], st["order"])
            for c, st in enumerate(pooled_statistics_gpu(cases, channels))}


def intensity_statistics_cpu(cases, channels):
    """The same definitions in numpy float64 on the pooled foreground values (host memory: 4 bytes per foreground voxel)."""
    out, pooled = {}, [[] for _ in range(channels)]
    for index, data, seg in cases.scan():
        for c in range(channels):
            values = data[c][seg > 0]
            if not np.isfinite(values).all():
                raise _nonfinite_error(cases.name(index), c)
            pooled[c].append(values)
    for c in range(channels):
        x = np.concatenate(pooled[c])
        if x.size == 0:
            raise _no_foreground_error(c)
        x64 = x.astype(np.float64)
        total = float(x64.sum())
        mean = total / x.size
        ranks = sorted({r for lo, hi, _ in quantile_ranks(x.size) for r in (lo, hi)})
        keys = np.partition(float_key(x), ranks)           # by key, so that -0.0 sorts before +0.0 as on the device
        order = {r: key_to_float(keys[r]) for r in ranks}
        out[str(c)] = finish_statistics(int(x.size), x.min(), x.max(), total, float(((x64 - mean) ** 2).sum()), order)
    return out


# ------------------------------------------------------------------------------------------------ the fingerprint
def extract_fingerprint(raw_dataset_dir, dataset_json, device="cuda", cache_bytes=DEFAULT_CACHE_BYTES, output_file=None):
    """The dict of dataset_fingerprint.json for the training cases of `raw_dataset_dir` (imagesTr / labelsTr), with nnU-Net's
    keys: foreground_intensity_properties_per_channel, median_relative_size_after_cropping, shapes_after_crop, spacings.
    The intensity values are exact over all foreground voxels (nnU-Net's are a sampled estimate of the same quantities).
    cache_bytes: device memory that cropped cases may occupy between the sweeps (not used on "cpu", which reads every case
    once); the result does not depend on it.  output_file: where to write the JSON (optional)."""
    listing = training_cases(raw_dataset_dir, dataset_json)
    channels = len(listing[0][1])
    cases = _Cases(listing, device, cache_bytes)
    stats = intensity_statistics_gpu(cases, channels) if cases.gpu else intensity_statistics_cpu(cases, channels)
    fingerprint = {
        "foreground_intensity_properties_per_channel": stats,
        "median_relative_size_after_cropping": float(np.median(cases.relative_sizes, 0)),
        "shapes_after_crop": cases.shapes,
        "spacings": cases.spacings,
    }
    if output_file is not None:
        Path(output_file).parent.mkdir(parents=True, exist_ok=True)
        with open(output_file, "w") as f:
            json.dump(fingerprint, f, indent=4, sort_keys=True)
    return fingerprint
