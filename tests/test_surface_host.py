"""CPU: the host side of the surface-distance entry points (csrc/surface.hip) without a device: the 64-bit workspace query and the
argument checks that must answer before anything is launched, and that the plan template stays the reference's schema."""
import ctypes

import pytest


def test_edt_size_query_and_argument_checks_need_no_device():
    from dg_tta_amd import _lib
    lib = _lib.load()
    assert lib.dgtta_edt_ws_bytes(16384, 16384, 16384) == 4 * 16384 ** 3          # computed in 64 bits
    assert lib.dgtta_edt_ws_bytes(0, 5, 5) == 0 and lib.dgtta_edt_ws_bytes(3, 5, 7) >= 3 * 5 * 7 * 4
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below is rejected by the checks in front of the launch
    assert lib.dgtta_edt_sq(None, None, None, 0, 4, 4, 4, 1.0, 1.0, 1.0, None) == -1
    assert lib.dgtta_edt_sq(fake, fake, fake, 1 << 30, 1025, 1, 1, 1.0, 1.0, 1.0, None) == -2
    assert b"at most 1024" in lib.dgtta_last_error()
    assert lib.dgtta_edt_sq(fake, fake, fake, 1 << 30, 4, 4, 4, 1.0, 0.0, 1.0, None) == -1
    assert lib.dgtta_edt_sq(fake, fake, fake, 16, 4, 4, 4, 1.0, 1.0, 1.0, None) == -3
    assert lib.dgtta_label_bboxes(fake, fake, 4, 4, 4, 1025, fake, None) == -2
    assert lib.dgtta_label_bboxes(fake, fake, 4, 4, 4, 0, fake, None) == -1
    assert lib.dgtta_label_surface(fake, 4, 4, 4, 1, 0, 0, 1, 4, 4, 4, fake, None) == -1
    assert b"outside" in lib.dgtta_last_error()


def test_surface_plan_keys_are_not_part_of_the_plan_template():
    from dg_tta_amd.tta.config_log_utils import TEMPLATE_PLAN
    assert not [k for k in TEMPLATE_PLAN if k.startswith("evaluation_")]


def test_array_spacing_reverses_pixdim():
    from dg_tta_amd.tta.evaluation import array_spacing
    assert array_spacing(None) == (1.0, 1.0, 1.0)
    assert array_spacing({"pixdim": (1.25, 0.75, 3.0)}) == (3.0, 0.75, 1.25)
