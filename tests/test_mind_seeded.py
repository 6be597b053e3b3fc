"""Seeded in-kernel MIND noise, the parts that need no GPU: the numpy restatement of the definition against Random123's
known answers and the worked example of include/dgtta.h, the two C entry points, and the host logic of the opt-in."""
import numpy as np
import pytest
import torch

import philox_ref


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    f = 0xFFFFFFFF
    assert _hex(philox_ref.philox4x32_10(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(philox_ref.philox4x32_10(f, f, f, f, f, f)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(philox_ref.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_worked_example():
    """seed 20240704, offset 0, b 0, channels 4..7, v = 5."""
    assert _hex(philox_ref.philox4x32_10(5, 1, 0, 0, 20240704, 0)) == "c90a4a0e 64caf89c 521f79ed 911947d0"
    n = philox_ref.mind_noise(20240704, 0, 0, 1, 2, 2, 8)
    assert np.allclose(n[0, 4:8, 0, 0, 5], [-0.54590064, 0.43050846, -1.37709972, -0.61442368], rtol=0, atol=5e-9)
    # the value belongs to (seed, offset, b, c, v): another volume shape with the same linear voxel index, another b0 split
    assert np.array_equal(philox_ref.mind_noise(20240704, 0, 0, 1, 1, 1, 6)[0, :, 0, 0, 5], n[0, :, 0, 0, 5])
    two = philox_ref.mind_noise(20240704, 3, 0, 2, 2, 3, 4)
    assert np.array_equal(two[1], philox_ref.mind_noise(20240704, 3, 1, 1, 2, 3, 4)[0])
    assert not np.array_equal(two[0], two[1])
    # both halves of seed and offset enter
    base = philox_ref.mind_noise(7, 1, 0, 1, 2, 2, 4)
    for seed, offset in ((7 + 2 ** 32, 1), (7, 1 + 2 ** 32), (8, 1), (7, 2)):
        assert not np.array_equal(philox_ref.mind_noise(seed, offset, 0, 1, 2, 2, 4), base)


def test_seeded_entry_points_are_exported_and_reject_null_arguments():
    from dg_tta_amd import _lib
    lib = _lib.load()
    assert "dgtta_mind3d_noise_fill" in _lib.SIGNATURES and "dgtta_mind3d_fwd_seeded" in _lib.SIGNATURES
    assert lib.dgtta_mind3d_noise_fill(None, 1, 0, 0, 1, 8, 8, 8, None) == -1
    assert b"mind3d_noise_fill: null pointer" in lib.dgtta_last_error()
    assert lib.dgtta_mind3d_noise_fill(None, 0, 0, 0, 0, 0, 0, 0, None) < 0 and lib.dgtta_last_error()
    taps = (_lib.F * 3)(0.25, 0.5, 0.25)
    assert lib.dgtta_mind3d_fwd_seeded(None, 1, 0, 0, 0.05, 1, taps, 3, None, 0, 12, 0, None, 0, 1, 8, 8, 8, None) == -1
    assert b"mind3d_fwd_seeded: null pointer" in lib.dgtta_last_error()
    assert lib.dgtta_mind3d_fwd_seeded(None, 0, 0, 0, 0.0, 0, None, 0, None, 0, 0, 0, None, 0, 0, 0, 0, 0, None) < 0
    assert lib.dgtta_last_error()
    # the checks that come before any launch hold for non-null pointers as well (nothing here touches a device)
    fake = 0x1000
    assert lib.dgtta_mind3d_noise_fill(fake, 1, 0, -1, 1, 8, 8, 8, None) == -1 and b"b0" in lib.dgtta_last_error()
    assert lib.dgtta_mind3d_noise_fill(fake, 1, 0, 0, 1, 2048, 1024, 1024, None) == -2
    assert lib.dgtta_mind3d_fwd_seeded(fake, 1, 0, 0, 0.05, 3, taps, 3, fake, 0, 12, 0, fake, 1 << 30, 1, 8, 8, 8, None) == -2
    assert lib.dgtta_mind3d_fwd_seeded(fake, 1, 0, 0, 0.05, 1, taps, 3, fake, 0, 12, 0, fake, 16, 1, 8, 8, 8, None) == -3
    # the tensor entry point still wants its noise
    assert lib.dgtta_mind3d_fwd(fake, None, 0.05, 1, taps, 3, fake, 0, 12, 0, fake, 1 << 30, 1, 8, 8, 8, None) == -1


def test_ops_take_exactly_one_noise_source_and_no_cpu_tensors():
    from dg_tta_amd import ops
    from dg_tta_amd._lib import DgttaError
    img = torch.zeros(1, 1, 8, 8, 8)
    with pytest.raises(ValueError, match="exactly one"):
        ops.mind3d(img)
    with pytest.raises(ValueError, match="exactly one"):
        ops.mind3d(img, torch.zeros(1, 12, 8, 8, 8), seed=3)
    with pytest.raises(DgttaError):
        ops.mind3d(img, seed=3)
    with pytest.raises(DgttaError):
        ops.mind3d_noise(1, 8, 8, 8, seed=3, device="cpu")


def test_kernel_noise_counts_calls_and_nests(monkeypatch):
    """Inside kernel_noise a call without a noise tensor goes to the seeded kernel with offset = its rank in the context and
    b0 = 0; a call WITH a tensor, and any call outside, is today's; contexts nest and an inner one does not advance the outer."""
    from dg_tta_amd import mind as hmind, ops
    seen = []

    def fake(img, noise=None, *a, seed=None, offset=0, b0=0, groups=1, **kw):
        seen.append(("tensor" if noise is not None else "seed", seed, offset, b0, groups))
        return torch.zeros(img.shape[0], *img.shape[2:], 16)

    monkeypatch.setattr(ops, "mind3d", fake)
    x, nz = torch.zeros(2, 1, 4, 4, 4), torch.zeros(2, 12, 4, 4, 4)
    m = hmind.MIND3D()
    state = torch.get_rng_state()
    with hmind.kernel_noise(11) as outer:
        m(x)
        m(x, nz)
        hmind.mind_hook(None, (x,))
        with hmind.kernel_noise(2 ** 64 + 5):
            m(x, groups=2)
        m(x)
        assert outer.calls == 3
    assert torch.equal(torch.get_rng_state(), state)             # nothing was drawn
    assert not hmind._KERNEL_NOISE
    m(x)                                                          # outside: the randn tensor
    assert seen == [("seed", 11, 0, 0, 1), ("tensor", None, 0, 0, 1), ("seed", 11, 1, 0, 1), ("seed", 5, 0, 0, 2),
                    ("seed", 11, 2, 0, 1), ("tensor", None, 0, 0, 1)]
    assert not torch.equal(torch.get_rng_state(), state)
    with pytest.raises(RuntimeError):
        with hmind.kernel_noise(1):
            raise RuntimeError("x")
    assert not hmind._KERNEL_NOISE


def test_plan_key_inference_mind_noise():
    import contextlib
    from dg_tta_amd import mind as hmind
    from dg_tta_amd.tta import config_log_utils as clu
    from dg_tta_amd.tta.tta import _inference_noise
    assert "inference_mind_noise" not in clu.TEMPLATE_PLAN
    assert isinstance(_inference_noise({}, 0), contextlib.nullcontext)
    assert isinstance(_inference_noise({"inference_mind_noise": "tensor", "seed": 3}, 0), contextlib.nullcontext)
    with pytest.raises(ValueError, match="inference_mind_noise"):
        _inference_noise({"inference_mind_noise": "philox"}, 0)
    a = _inference_noise({"inference_mind_noise": "kernel", "seed": 3}, 0)
    b = _inference_noise({"inference_mind_noise": "kernel", "seed": 3}, 1)
    c = _inference_noise({"inference_mind_noise": "kernel", "seed": 4}, 0)
    assert all(isinstance(k, hmind.kernel_noise) for k in (a, b, c)) and len({a.seed, b.seed, c.seed}) == 3
    assert a.seed == _inference_noise({"inference_mind_noise": "kernel", "seed": 3}, 0).seed
    state = torch.get_rng_state()
    d = _inference_noise({"inference_mind_noise": "kernel"}, 2)          # no plan seed: torch.initial_seed()
    assert d.seed == (torch.initial_seed() + 0x9E3779B97F4A7C15 * 3) % 2 ** 64 and torch.equal(torch.get_rng_state(), state)
