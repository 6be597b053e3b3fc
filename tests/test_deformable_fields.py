"""Host tests of spatial_aug_type="deformable": the torch restatement (tests/deformable_ref.py) against the fixtures written
from the reference's own functions, and the host-side behaviour of the product up to its first device call."""
import types

import pytest
import torch

import deformable_ref as dref
from conftest import load_golden


def _fixture():
    g, gl = load_golden("deformable"), load_golden("deformable_logits")
    return g, gl, [int(v) for v in g["size"]]


def test_fp32_restatement_reproduces_the_reference_bit_for_bit():
    g, gl, size = _fixture()
    assert len(set(size)) == 3 and min(size) >= 25           # non-cubic: a transposed axis cannot pass
    field = dref.rf_field(g["draw"], size)
    assert torch.equal(field, g["field"])
    disp, inv = dref.diffeo_fields(field)
    assert torch.equal(disp, g["disp"]) and torch.equal(inv, g["inverse"])
    image = dref.hash_noise([1, 1] + size, 1).float()
    assert torch.equal(dref.dense_warp(image, disp, "border"), g["image_warped"])
    logits = dref.hash_noise([1, 5] + size, 2).float()
    weight = dref.hash_noise([1, 5] + size, 3).float()
    out, grad = dref.warp_and_grad(logits, inv, weight)
    assert torch.equal(out, gl["logits_warped"]) and torch.equal(grad, gl["logits_grad"])
    assert 0.01 < float(disp.abs().max()) < 0.5          # a displacement of a few voxels, in normalised grid units


def test_fp64_restatement_is_close_to_fp32():
    g, _, size = _fixture()
    f64 = dref.rf_field(g["draw"].double(), size)
    assert float((f64 - g["field"]).abs().max()) < 1e-4
    d64, i64 = dref.diffeo_fields(f64)
    assert float((d64 - g["disp"]).abs().max()) < 1e-5 and float((i64 - g["inverse"]).abs().max()) < 1e-5


@pytest.mark.parametrize("size", [[24, 32, 32], [32, 24, 40], [40, 32, 24]])
def test_patch_axis_below_25_is_rejected_on_the_host(size):
    from dg_tta_amd.tta.augmentation_utils import get_disp_field
    with pytest.raises(ValueError, match="25"):
        get_disp_field(1, size, factor=0.5, interpolation_factor=5)          # before any tensor or launch


def test_even_interpolation_factor_is_not_offered():
    from dg_tta_amd.tta.augmentation_utils import get_rf_field
    with pytest.raises(NotImplementedError):
        get_rf_field(1, [32, 32, 32], interpolation_factor=4)


def _host_config(**kw):
    return dict(dict(have_grad_in="both", do_intensity_aug_in="none", do_spatial_aug_in="both",
                     spatial_aug_type="deformable"), **kw)


def test_plan_value_deformable_reaches_the_device_layer():
    """On a machine without a GPU the deformable plan runs through the host path and stops where the first kernel would be
    launched (there is no CPU fallback), not at a NotImplementedError; both entry points."""
    from dg_tta_amd._lib import DgttaError
    from dg_tta_amd.tta import tta
    mods = types.SimpleNamespace(ModifierFunctions=types.SimpleNamespace(modify_tta_output_after_mapping_fn=lambda x: x))
    model = torch.nn.Identity()
    imgs = torch.zeros(1, 1, 25, 30, 35)
    with pytest.raises(DgttaError, match="no CPU fallback"):
        tta.calc_branch("branch_a", _host_config(), model, lambda x: x, None, [25, 30, 35], 1, None, [0, 1], mods, imgs, "cpu")
    with pytest.raises(DgttaError, match="no CPU fallback"):
        tta.prepare_both_branches(_host_config(), model, lambda x: x, 1, imgs, "cpu", steps=2)
    with pytest.raises(ValueError, match="25"):
        tta.prepare_both_branches(_host_config(), model, lambda x: x, 1, torch.zeros(1, 1, 24, 32, 32), "cpu")


def test_new_abi_calls_check_their_arguments_without_a_device():
    from dg_tta_amd import _lib
    lib = _lib.load()
    assert lib.dgtta_rf_field_ws_bytes(3, 5, 6, 7) >= 2 * 3 * 5 * 6 * 7 * 4
    assert lib.dgtta_diffeo_fields_ws_bytes(2, 25, 30, 35) >= 2 * 25 * 30 * 35 * 3 * 4 * 2
    assert lib.dgtta_rf_field_fwd(None, None, None, 0, 3, 5, 5, 6, 7, 25, 30, 35, None) == -1
    assert b"null pointer" in lib.dgtta_last_error()
    one = 256                                        # any non-null address: rejected before it is touched
    assert lib.dgtta_rf_field_fwd(one, one, one, 1 << 30, 3, 5, 4, 6, 7, 24, 30, 35, None) == -1
    assert b"smaller than" in lib.dgtta_last_error()
    assert lib.dgtta_rf_field_fwd(one, one, one, 1 << 30, 3, 4, 6, 6, 7, 24, 30, 35, None) == -2
    assert lib.dgtta_rf_field_fwd(one, one, one, 16, 3, 5, 5, 6, 7, 25, 30, 35, None) == -3
    assert lib.dgtta_diffeo_fields(one, 0.5, one, one, one, 16, 1, 25, 30, 35, 5, None) == -3
    assert lib.dgtta_diffeo_fields(one, 0.5, one, one, one, 1 << 30, 1, 25, 30, 35, 0, None) == -1
    assert lib.dgtta_dense_warp3d_fwd(one, one, one, 1, 5, 25, 30, 35, 1, 4, 5, 0, None) == -1
    assert b"ldc" in lib.dgtta_last_error()
    assert lib.dgtta_dense_warp3d_bwd(one, one, one, 1, 5, 25, 30, 35, 0, 0, 0, 7, None) == -1
    assert b"pad_mode" in lib.dgtta_last_error()
