"""GPU: extract_fingerprint on a five-case synthetic dataset.  With nothing resident (cache_bytes = 0: every case is read from
disk again in sweeps 2 and 3) and with everything resident it writes byte-identical JSON; both equal the device="cpu" path
(numpy float64 on the pooled foreground values) in shapes, spacings, min, max and the percentiles' order statistics exactly,
and in mean / std within the bounds of tests/test_gpu_fingerprint.py.  The dataset has two channels and cases whose
cropped voxel count is no multiple of four (35 x 31 x 41, 25 x 31 x 37): every channel is cut into a tensor of its own."""
import json

import numpy as np
import pytest

from fingerprint_ref import moment_bounds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(40, 36, 44), (33, 48, 40), (44, 44, 44), (25, 31, 37), (48, 40, 36)]
SPACINGS = [(1.0, 1.0, 2.5), (0.8, 0.8, 3.0), (1.5, 1.5, 1.5), (0.75, 0.75, 2.0), (1.0, 1.25, 2.5)]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from dg_tta_amd.tta.nifti_io import write_nifti
    raw = tmp_path_factory.mktemp("raw") / "Dataset812_Fingerprint"
    (raw / "imagesTr").mkdir(parents=True)
    (raw / "labelsTr").mkdir()
    rng = np.random.default_rng(23)
    pooled = [[], []]
    for i, (shape, spacing) in enumerate(zip(SHAPES, SPACINGS)):
        img = rng.integers(-1000, 1500, shape).astype(np.float32)
        img[img == 0] = 1.0
        if i % 2 == 0:                                       # a zero border that the crop removes
            inner = np.zeros_like(img)
            inner[2:-3, 4:-1, 1:-2] = img[2:-3, 4:-1, 1:-2]
            img = inner
        lab = np.zeros(shape, dtype=[np.uint8, np.int16, np.int32][i % 3])
        lab[5:-6, 6:-5, 4:-8] = 1
        lab[8:14, 9:15, 7:16] = 2
        if i == 3:
            lab[:] = 0                                       # a case without foreground
        second = np.where(img != 0, img * np.float32(0.5) + np.float32(7.25), 0).astype(np.float32)
        write_nifti(raw / "imagesTr" / f"case{i}_0000.nii.gz", img, spacing=spacing)
        write_nifti(raw / "imagesTr" / f"case{i}_0001.nii.gz", second, spacing=spacing)
        write_nifti(raw / "labelsTr" / f"case{i}.nii.gz", lab, spacing=spacing)
        pooled[0].append(img[lab > 0])
        pooled[1].append(second[lab > 0])
    dataset_json = {"labels": {"background": 0, "a": 1, "b": 2}, "file_ending": ".nii.gz", "channel_names": {"0": "CT", "1": "T1"},
                    "numTraining": 5}
    return raw, dataset_json, [np.concatenate(p) for p in pooled]


def test_the_result_does_not_depend_on_the_cache_budget(dataset, tmp_path):
    from dg_tta_amd.planning.fingerprint import extract_fingerprint, quantile_ranks
    raw, dataset_json, pooled = dataset
    streamed = extract_fingerprint(raw, dataset_json, device=DEV, cache_bytes=0, output_file=tmp_path / "streamed.json")
    resident = extract_fingerprint(raw, dataset_json, device=DEV, cache_bytes=2 ** 30, output_file=tmp_path / "resident.json")
    half = extract_fingerprint(raw, dataset_json, device=DEV, cache_bytes=600000, output_file=tmp_path / "half.json")
    assert (tmp_path / "streamed.json").read_bytes() == (tmp_path / "resident.json").read_bytes() == (tmp_path / "half.json").read_bytes()
    assert streamed == resident == half == json.load(open(tmp_path / "streamed.json"))

    host = extract_fingerprint(raw, dataset_json, device="cpu")
    assert resident["shapes_after_crop"] == host["shapes_after_crop"] and resident["spacings"] == host["spacings"]
    assert resident["shapes_after_crop"][0] == [35, 31, 41] and resident["shapes_after_crop"][1] == list(SHAPES[1])
    assert resident["spacings"] == [[float(np.float32(s)) for s in sp[::-1]] for sp in SPACINGS]
    assert resident["median_relative_size_after_cropping"] == host["median_relative_size_after_cropping"] < 1.0
    for channel in ("0", "1"):
        got, want = resident["foreground_intensity_properties_per_channel"][channel], host["foreground_intensity_properties_per_channel"][channel]
        # the percentiles are the same three double operations on the same exact order statistics in both paths
        for key in ("min", "max", "median", "percentile_00_5", "percentile_99_5"):
            assert got[key] == want[key], key
        x = np.sort(pooled[int(channel)].astype(np.float64))
        n = x.size
        for key, (lo, hi, frac) in zip(("percentile_00_5", "median", "percentile_99_5"), quantile_ranks(n)):
            assert got[key] == x[lo] + (x[hi] - x[lo]) * frac
        # the depth bounds of tests/test_gpu_fingerprint.py (fingerprint_ref.moment_bounds), inside the a-priori ones
        mean_bound, std_bound = moment_bounds(x, [int(np.prod(s)) for s in resident["shapes_after_crop"]])
        print(f"\nchannel {channel}: mean error {abs(got['mean'] - x.mean()):.3e} (bound {mean_bound:.3e}), std error {abs(got['std'] - x.std()):.3e} "
              f"(bound {std_bound:.3e})")
        assert abs(got["mean"] - x.mean()) <= min(mean_bound, n * 2.0 ** -53 * np.abs(x).mean())
        assert abs(got["std"] - x.std()) <= min(std_bound, 4 * n * 2.0 ** -53 * np.abs(x - x.mean()).max())
        assert abs(want["mean"] - x.mean()) <= min(mean_bound, n * 2.0 ** -53 * np.abs(x).mean())
        assert abs(want["std"] - x.std()) <= std_bound
