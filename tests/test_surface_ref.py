"""CPU: licenses tests/surface_ref.py (the float64 reference of the surface-distance kernels) against scipy.ndimage on the same
table of cases the GPU tests use: the surface against binary_erosion, the brute-force squared distances against
distance_transform_edt(sampling=...), the metrics against the definitions evaluated with scipy's transform."""
import numpy as np
import pytest

ndi = pytest.importorskip("scipy.ndimage")

import surface_ref as sref  # noqa: E402


@pytest.mark.parametrize("shape", sref.EDT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edt_sq_matches_scipy(shape):
    for kind in sref.EDT_SITES:
        site = sref.site_mask(shape, kind)
        for spacing in sref.SPACINGS:
            got = sref.edt_sq(site, spacing)
            if not site.any():
                assert np.all(np.isposinf(got))
                continue
            want = ndi.distance_transform_edt(~site, sampling=sref.f32_spacing(spacing)) ** 2
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=f"{kind} {spacing}")
        if site.any():
            exact = sref.edt_sq_int(site)
            assert np.array_equal(exact, np.round(exact)) and np.array_equal(exact.astype(np.float64), sref.edt_sq(site))
        if kind == "all":
            assert not sref.edt_sq(site).any()


@pytest.mark.parametrize("shape", sref.EDT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_surface_matches_binary_erosion(shape):
    for kind in sref.EDT_SITES:
        m = sref.site_mask(shape, kind)
        assert np.array_equal(sref.surface(m), m & ~ndi.binary_erosion(m, border_value=0)), kind


def test_surface_of_the_synthetic_pair_matches_binary_erosion():
    ref, pred = sref.synthetic_pair()
    for a in (ref, pred):
        for l in sref.PAIR_LABELS:
            m = a == l
            assert np.array_equal(sref.surface(m), m & ~ndi.binary_erosion(m, border_value=0))


@pytest.mark.parametrize("spacing", sref.SPACINGS[:2])
def test_metrics_match_the_definitions_evaluated_with_scipy(spacing):
    ref, pred = sref.synthetic_pair()
    s = sref.f32_spacing(spacing)
    for l in (1, 2, 3):
        sp, sr = sref.surface(pred == l), sref.surface(ref == l)
        d_rp = ndi.distance_transform_edt(~sp, sampling=s)[sr]
        d_pr = ndi.distance_transform_edt(~sr, sampling=s)[sp]
        both = np.concatenate([d_rp, d_pr])
        m = sref.metrics(pred, ref, l, spacing, tau=1.5)
        assert m["HD95"] == pytest.approx(np.percentile(both, 95), rel=1e-12, abs=0)
        assert m["HD"] == pytest.approx(both.max(), rel=1e-12, abs=0)
        assert m["ASSD"] == pytest.approx((d_rp.mean() + d_pr.mean()) / 2, rel=1e-12, abs=0)
        assert m["NSD"] == ((d_rp <= 1.5).sum() + (d_pr <= 1.5).sum()) / both.size


def test_synthetic_pair_sanity_values():
    ref, pred = sref.synthetic_pair()
    m = {l: sref.metrics(pred, ref, l) for l in sref.PAIR_LABELS}
    assert m[1]["HD95"] == pytest.approx(np.sqrt(5.0), rel=1e-12)
    assert m[2]["HD"] == pytest.approx(15.62, abs=0.005)
    assert m[3] == {"HD95": 0.0, "HD": 0.0, "ASSD": 0.0, "NSD": 1.0}
    assert m[4] == {"HD95": np.inf, "HD": np.inf, "ASSD": np.inf, "NSD": 0.0}
    assert all(np.isnan(v) for v in m[5].values())
    assert sref.metrics(pred, ref, 2, (3.0, 0.75, 1.25))["HD"] == pytest.approx(24.19, abs=0.005)
    assert sref.metrics(pred, ref, 2, (1.25, 0.75, 3.0))["HD"] != pytest.approx(24.19, abs=0.005)      # swapped axes differ
    boxes = sref.bboxes(ref, pred, 6)
    assert boxes[5] is None and boxes[4] == (10, 12, 16, 10, 12, 16) and boxes[3] == (0, 0, 0, 0, 0, 16)


def test_nsd_tau_is_away_from_every_distance():
    ref, pred = sref.synthetic_pair()
    for spacing in sref.SPACINGS[:2]:
        tau, half = sref.nsd_tau(pred, ref, sref.PAIR_LABELS, spacing)
        assert 1.0 < tau < 3.0 and half > 1e-3
