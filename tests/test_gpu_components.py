"""GPU: the connected-component kernels of csrc/components.hip (dgtta_cc_label, dgtta_cc_sizes, dgtta_cc_filter) and the
post-processing built on them (dg_tta_amd/tta/postprocessing.py, the hook of run_tta) against the numpy reference
tests/components_ref.py, which tests/test_components_ref.py licenses against scipy.ndimage.label.  No scipy here.

Everything is integer valued and canonical (a component is named by its smallest linear index), so every comparison is exact
equality on every voxel; there is no tolerance and nothing is left out.

Shapes: the kernels label tiles of 8 x 8 x 64 voxels (D, H, W) in LDS and unite them across tile borders afterwards, so each axis
has to appear one below, one above and one above twice its tile extent.  The issue's list - (1,1,1), (1,1,130), (2,3,5), (7,9,65),
(9,17,33), (17,33,129) - has D at 7 / 9 / 17, H at 9 / 17 and W at 65 / 129; (3,7,63) is added for H = 7 and W = 63."""
import ctypes

import numpy as np
import pytest
import torch

import components_ref as R
import surface_ref as sref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)        # a copy: the shared inputs are read-only


def _gpu_cc(seg, table, connectivity):
    from dg_tta_amd import ops
    cc = ops.cc_label(_dev(seg), _dev(table), connectivity)
    return cc, ops.cc_sizes(cc)


def _check_cc(seg, table, connectivity, want=None, where=""):
    cc, size = _gpu_cc(seg, table, connectivity)
    cc2, size2 = _gpu_cc(seg, table, connectivity)
    assert cc.dtype == torch.int32 and cc.shape == seg.shape and size.dtype == torch.int32 and size.shape == (seg.size,)
    assert torch.equal(cc, cc2) and torch.equal(size, size2), f"{where}: two runs differ"
    want_cc = R.label(seg, table, connectivity) if want is None else want[0]
    want_size = R.sizes(want_cc) if want is None else want[1]
    bad = np.flatnonzero(cc.cpu().numpy().reshape(-1) != want_cc.reshape(-1))
    assert bad.size == 0, f"{where}: cc differs at {bad.size} voxels, first {bad[:5]}"
    bad = np.flatnonzero(size.cpu().numpy() != want_size)
    assert bad.size == 0, f"{where}: size differs at {bad.size} roots, first {bad[:5]}"


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_cc_and_sizes_vs_reference(shape, connectivity):
    """All background, all one label, the checkerboard, two labels in face contact (apart as two groups, merged as one), the
    serpentine, and noise at p = 0.2 / 0.31 / 0.5 with one and with five labels, each label its own group and all in one."""
    for kind in R.GENERIC_KINDS:
        for table_name, table in (("own", R.own_groups(5)), ("one", R.one_group(5))):
            _check_cc(R.volume(kind, shape), table, connectivity, R.reference(kind, shape, table_name, 5, connectivity),
                      f"{kind} {shape} {table_name} c{connectivity}")


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_special_inputs_vs_reference(connectivity):
    """Edge-only and corner-only contact across a tile corner, the U's whose arms meet in the next tile, the tie volume, a table
    with regions, unused and out-of-range entries, labels outside the table (negative ones too)."""
    for name, seg in (("edge", R.contact_pair("edge")), ("corner", R.contact_pair("corner")), ("u", R.u_shapes()), ("tie", R.tie_volume())):
        _check_cc(seg, R.own_groups(5), connectivity, where=f"{name} own c{connectivity}")
        _check_cc(seg, R.one_group(5), connectivity, where=f"{name} one c{connectivity}")
    seg = R.volume("noise0.5x5", (9, 17, 33)).copy()
    seg[0, 0, :4] = [-1, -7, 6, 2 ** 40]
    _check_cc(seg, np.array([0, 2, 0, 2, 1, 7], dtype=np.int32), connectivity, where="regions")
    _check_cc(seg, np.array([0, 2, 0, 2, -3, 1], dtype=np.int32), connectivity, where="negative entry")
    _check_cc(seg, np.array([1, 0, 0], dtype=np.int32), connectivity, where="background as the only group")


def test_known_component_counts():
    def count(seg, table, c):
        return int(torch.count_nonzero(_gpu_cc(seg, table, c)[1]))
    board = R.volume("checkerboard", (4, 4, 4))
    assert [count(board, R.own_groups(1), c) for c in R.CONNECTIVITIES] == [32, 1, 1]
    assert [count(R.contact_pair("edge"), R.own_groups(1), c) for c in R.CONNECTIVITIES] == [2, 1, 1]
    assert [count(R.contact_pair("corner"), R.own_groups(1), c) for c in R.CONNECTIVITIES] == [2, 2, 1]
    halves = R.volume("halves", (9, 17, 33))
    assert count(halves, R.own_groups(2), 6) == 2 and count(halves, R.one_group(2), 6) == 1
    assert all(count(R.u_shapes(), R.own_groups(3), c) == 3 for c in R.CONNECTIVITIES)


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("p", ["0.2", "0.31", "0.5"])
def test_noise_near_the_percolation_threshold(p, connectivity):
    """33 x 34 x 70: thousands of tangled components that cross every tile border, the hard case for a union-find."""
    _check_cc(R.volume(f"noise{p}x1", R.NOISE_SHAPE), R.own_groups(1), connectivity, where=f"p={p} 1 label")
    _check_cc(R.volume(f"noise{p}x5", R.NOISE_SHAPE), R.own_groups(5), connectivity, where=f"p={p} 5 labels")


FILTER_SETTINGS = [(True, 0, 0), (False, 5, 0), (True, 4, 7), (False, 0, 0)]


def _check_filter(seg, table, connectivity, keep_largest, min_voxels, background, where):
    from dg_tta_amd import ops
    m, t = _dev(seg), _dev(table)
    cc = ops.cc_label(m, t, connectivity)
    size = ops.cc_sizes(cc)
    out, removed = ops.cc_filter(m, t, cc, size, keep_largest, min_voxels, background)
    out2, removed2 = ops.cc_filter(m, t, cc, size, keep_largest, min_voxels, background)
    assert torch.equal(out, out2) and torch.equal(removed, removed2), f"{where}: two runs differ"
    want_out, want_removed = R.filter_map(seg, table, connectivity, keep_largest, min_voxels, background)
    assert out.dtype == torch.int64 and removed.dtype == torch.int64
    assert np.array_equal(out.cpu().numpy(), want_out), where
    assert np.array_equal(removed.cpu().numpy(), want_removed), where
    assert torch.equal(m, _dev(seg))            # the input is left alone


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("keep_largest,min_voxels,background", FILTER_SETTINGS)
def test_filter_vs_reference(connectivity, keep_largest, min_voxels, background):
    cases = [(R.tie_volume(), R.own_groups(4)), (R.tie_volume(), np.array([0, 1, 2, 2, 3], dtype=np.int32)),
             (R.volume("noise0.31x5", R.NOISE_SHAPE), R.own_groups(5)), (R.volume("noise0.2x5", (7, 9, 65)), R.one_group(5)),
             (R.volume("noise0.5x5", (9, 17, 33)), np.array([0, 2, 0, 2, 1, 7], dtype=np.int32)),
             (R.volume("serpentine", (17, 33, 129)), R.own_groups(1)), (R.volume("background", (2, 3, 5)), R.own_groups(1)),
             (R.volume("solid", (1, 1, 1)), R.own_groups(3))]
    for k, (seg, table) in enumerate(cases):
        _check_filter(seg, table, connectivity, keep_largest, min_voxels, background, f"case {k}")


def test_tie_and_threshold_rules():
    from dg_tta_amd import ops
    seg = R.tie_volume()

    def run(table, **kw):
        m, t = _dev(seg), _dev(np.asarray(table, dtype=np.int32))
        cc = ops.cc_label(m, t, 26)
        out, removed = ops.cc_filter(m, t, cc, ops.cc_sizes(cc), **kw)
        return out.cpu().numpy(), removed.cpu().tolist()
    out, removed = run(R.own_groups(4))
    assert (out[0, 0, 0:3] == 1).all() and (out[2, 2, 65:68] == 0).all()          # equal sizes: the first component stays
    assert removed == [0, 3, 0, 0, 4]
    out, removed = run([0, 0, 1, 1, 0])
    assert (out[1, 4, 10:14] == 3).all() and (out[3, 4, 60:64] == 0).all()        # labels 2 and 3 as one region tie as well
    assert removed == [0, 4, 0, 0, 0]
    out, removed = run(R.own_groups(4), keep_largest=False, min_voxels=5)
    assert (out[0, 6, 30:35] == 4).all() and np.count_nonzero(out) == 5           # exactly min_voxels stays, one below goes
    assert removed == [0, 6, 4, 4, 4]


def test_caller_buffers_are_used_and_checked():
    from dg_tta_amd import ops
    seg, table = R.volume("noise0.31x5", (7, 9, 65)), R.own_groups(5)
    m, t = _dev(seg), _dev(table)
    n = seg.size
    want_cc, want_size = R.reference("noise0.31x5", (7, 9, 65), "own", 5, 26)
    want_out, _ = R.filter_map(seg, table, 26)
    assert ops.cc_ws_bytes(*seg.shape) >= 4 * n and ops.cc_ws_bytes(1, 1, 1) >= 8 * 1024 and ops.cc_ws_bytes(0, 1, 1) == 0
    cc_buf = torch.full((n + 100,), -5, dtype=torch.int32, device=DEV)
    size_buf = torch.full((n + 100,), -5, dtype=torch.int32, device=DEV)
    out_buf = torch.full((n + 100,), -5, dtype=torch.int64, device=DEV)
    ws = torch.empty(ops.cc_ws_bytes(*seg.shape) + 64, dtype=torch.uint8, device=DEV)
    cc = ops.cc_label(m, t, 26, out=cc_buf, ws=ws)
    size = ops.cc_sizes(cc, out=size_buf)
    out, _ = ops.cc_filter(m, t, cc, size, out=out_buf, ws=ws)
    assert cc.data_ptr() == cc_buf.data_ptr() and size.data_ptr() == size_buf.data_ptr() and out.data_ptr() == out_buf.data_ptr()
    assert np.array_equal(cc.cpu().numpy(), want_cc) and np.array_equal(size.cpu().numpy(), want_size)
    assert np.array_equal(out.cpu().numpy(), want_out)
    for buf in (cc_buf, size_buf, out_buf):
        assert (buf[n:] == -5).all()            # nothing is written behind D*H*W elements
    for bad in (cc_buf.long(), cc_buf[:n - 1], cc_buf.cpu(), cc_buf[::2]):
        with pytest.raises(ValueError, match="cc_label: out"):
            ops.cc_label(m, t, 26, out=bad)
        with pytest.raises(ValueError, match="cc_sizes: out"):
            ops.cc_sizes(cc, out=bad)
    for bad in (out_buf.int(), out_buf[:n - 1], out_buf.cpu()):
        with pytest.raises(ValueError, match="cc_filter: out"):
            ops.cc_filter(m, t, cc, size, out=bad)
    for bad in (ws[:16], ws.cpu(), ws.view(torch.int32)):
        with pytest.raises(ValueError, match="cc_label: ws"):
            ops.cc_label(m, t, 26, ws=bad)
        with pytest.raises(ValueError, match="cc_filter: ws"):
            ops.cc_filter(m, t, cc, size, ws=bad)


def test_bad_arguments_raise():
    from dg_tta_amd import _lib, ops
    seg, table = R.volume("halves", (2, 3, 5)), R.own_groups(2)
    m, t = _dev(seg), _dev(table)
    cc = ops.cc_label(m, t, 26)
    size = ops.cc_sizes(cc)
    for bad in (m.int(), m[0], m.permute(2, 1, 0)):
        with pytest.raises(ValueError, match="int64 label map"):
            ops.cc_label(bad, t, 26)
    for bad in (t.long(), t[:0], torch.zeros(1025, dtype=torch.int32, device=DEV), t.cpu(), t.view(1, -1)):
        with pytest.raises(ValueError, match="group must be"):
            ops.cc_label(m, bad, 26)
        with pytest.raises(ValueError, match="group must be"):
            ops.cc_filter(m, bad, cc, size)
    with pytest.raises(_lib.DgttaError):
        ops.cc_label(m.cpu(), t, 26)
    for c in (0, 4, 8, 27):
        with pytest.raises(_lib.DgttaError, match="connectivity"):
            ops.cc_label(m, t, c)
    with pytest.raises(ValueError, match="int32 component map"):
        ops.cc_sizes(cc.long())
    with pytest.raises(ValueError, match="cc_filter: cc"):
        ops.cc_filter(m, t, cc.long(), size)
    with pytest.raises(ValueError, match="cc_filter: size"):
        ops.cc_filter(m, t, cc, size[:3])
    with pytest.raises(ValueError, match="min_voxels"):
        ops.cc_filter(m, t, cc, size, min_voxels=-1)
    # 2^31 - 1 voxels and more are refused before anything is launched or read: the buffers here are far too small
    lib = _lib.load()
    ws = torch.empty(256, dtype=torch.uint8, device=DEV)
    for d, h, w in ((2048, 1024, 1024), (1, 1, 2 ** 31 - 1)):
        rc = lib.dgtta_cc_label(m.data_ptr(), t.data_ptr(), 3, d, h, w, 26, cc.data_ptr(), ws.data_ptr(), ctypes.c_size_t(2 ** 40), None)
        assert rc == -2 and b"2^31" in lib.dgtta_last_error()
    assert lib.dgtta_cc_sizes(cc.data_ptr(), 2 ** 31 - 1, size.data_ptr(), None) == -2
    torch.cuda.synchronize()


def _noisy_prediction():
    """The prediction of surface_ref's pair with a one-voxel island of label 1 in a far corner, and two voxels of label 2."""
    ref, pred = sref.synthetic_pair()
    noisy = pred.copy()
    assert noisy[10, 0, 0] == 0 and noisy[0, 12, 0] == 0
    noisy[10, 0, 0] = 1
    noisy[0, 12, 0:2] = 2
    return ref, pred, noisy


def test_keep_largest_components_on_numpy_and_tensors():
    from dg_tta_amd.tta import postprocessing as pp
    _, pred, noisy = _noisy_prediction()
    got, removed = pp.keep_largest_components(noisy.astype(np.int16))
    assert isinstance(got, np.ndarray) and got.dtype == np.int16 and np.array_equal(got, pred)
    assert removed == {1: 1, 2: 2, 3: 0}                                 # None: the labels present, each on its own
    got, removed = pp.keep_largest_components(torch.from_numpy(noisy), [1, (2, 3)], connectivity=6)
    want, want_removed = R.filter_map(noisy, np.array([0, 1, 2, 2], dtype=np.int32), 6)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and got.device.type == "cpu"
    assert np.array_equal(got.numpy(), want) and removed == {1: int(want_removed[1]), (2, 3): int(want_removed[2])}
    got, removed = pp.keep_largest_components(torch.from_numpy(noisy).to(DEV, torch.int32), "foreground", min_voxels=3, background=9)
    want, want_removed = R.filter_map(noisy, R.one_group(1023), 26, True, 3, 9)
    assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert removed == {"foreground": int(want_removed[1])}
    got, removed = pp.keep_largest_components(noisy, [2], keep_largest=False, min_voxels=3)
    assert np.array_equal(got, R.filter_map(noisy, np.array([0, 0, 1], dtype=np.int32), 26, False, 3)[0]) and removed == {2: 2}
    got, removed = pp.keep_largest_components(np.zeros((2, 3, 4), dtype=np.uint8))
    assert not got.any() and removed == {}
    cc, size = pp.connected_components(noisy, connectivity=18)
    want_cc = R.label(noisy, R.own_groups(3), 18)
    assert isinstance(cc, np.ndarray) and cc.dtype == np.int32 and np.array_equal(cc, want_cc) and np.array_equal(size, R.sizes(want_cc))
    with pytest.raises(ValueError, match="call twice"):
        pp.keep_largest_components(noisy, [1, (1, 2)])
    with pytest.raises(ValueError, match="connectivity"):
        pp.keep_largest_components(noisy, [1], connectivity=8)
    with pytest.raises(ValueError, match="integer label map"):
        pp.keep_largest_components(noisy.astype(np.float32))


def test_nnunet_name_with_a_region_tuple():
    from dg_tta_amd.tta.postprocessing import remove_all_but_largest_component_from_segmentation as nnunet_fn
    _, _, noisy = _noisy_prediction()
    got = nnunet_fn(noisy, [(1, 2), 3], background_label=5)
    assert np.array_equal(got, R.filter_map(noisy, np.array([0, 1, 1, 2], dtype=np.int32), 26, background=5)[0])
    got = nnunet_fn(noisy, (1, 2))                                       # one region, not in a list
    assert np.array_equal(got, R.filter_map(noisy, np.array([0, 1, 1], dtype=np.int32), 26)[0])
    # entries that share a label are applied one by one, each to the original segmentation
    got = nnunet_fn(noisy, [(1, 2), 2])
    a = R.filter_map(noisy, np.array([0, 1, 1], dtype=np.int32), 26)[0]
    b = R.filter_map(noisy, np.array([0, 0, 1], dtype=np.int32), 26)[0]
    assert np.array_equal(got, np.where((a != noisy) | (b != noisy), 0, noisy))


def test_postprocess_prediction_follows_the_plan_keys(capsys):
    from dg_tta_amd.tta.tta import _postprocess_prediction
    _, pred, noisy = _noisy_prediction()
    seg = torch.from_numpy(noisy)
    names = ["background", "organ", "ball", "line"]
    assert _postprocess_prediction(seg, {"optimized_labels": names}, DEV) is seg
    got = _postprocess_prediction(seg, {"optimized_labels": names, "postprocessing_keep_largest_component": True}, DEV)
    assert got is not seg and got.dtype == seg.dtype and got.device == seg.device
    assert np.array_equal(got.numpy(), R.filter_map(noisy, R.own_groups(3), 26)[0]) and np.array_equal(got.numpy(), pred)
    assert "organ=1, ball=2, line=0" in capsys.readouterr().out
    got = _postprocess_prediction(seg, {"optimized_labels": names, "postprocessing_keep_largest_component": "foreground",
                                        "postprocessing_connectivity": 6}, DEV)
    assert np.array_equal(got.numpy(), R.filter_map(noisy, R.one_group(1023), 6)[0])
    got = _postprocess_prediction(seg, {"optimized_labels": names, "postprocessing_keep_largest_component": [["organ", 2], "line"]}, DEV)
    assert np.array_equal(got.numpy(), R.filter_map(noisy, np.array([0, 1, 1, 2], dtype=np.int32), 26)[0])
    assert "organ+ball=" in capsys.readouterr().out
    got = _postprocess_prediction(seg, {"optimized_labels": names, "postprocessing_min_component_voxels": 2}, DEV)
    assert np.array_equal(got.numpy(), R.filter_map(noisy, R.own_groups(3), 26, False, 2)[0])
    assert torch.equal(seg, torch.from_numpy(noisy))


def test_run_tta_writes_the_filtered_prediction(tmp_path, monkeypatch):
    """tta_main with `postprocessing_keep_largest_component: true` on one synthetic case: the written prediction equals the
    reference filter applied to the unfiltered one, and the summary counts the filtered file."""
    import json
    from types import SimpleNamespace as NS

    from conftest import load_golden
    from test_gpu_tta import _network_with_hooks, _plan, _synthetic_case

    from dg_tta_amd.tta import tta as tta_mod
    from dg_tta_amd.tta.config_log_utils import ModifierFunctions
    net = _network_with_hooks(load_golden("calc_branch"))
    cfg = _plan(epochs=1, ensemble_count=1, patches_to_be_accumulated=2, tta_data_filepaths=[], seed=3,
                pretrained_weights_filepath="unused", lr=1e-4)
    cfg["optimized_labels"] = ["background", "a", "b", "c"]
    cfg["postprocessing_keep_largest_component"] = True
    mapping = {"background": (0, 0), "a": (2, 1), "b": (3, 2), "c": (5, 3)}
    seen, hook = [], tta_mod._postprocess_prediction

    def spy(seg, config, device):
        out = hook(seg, config, device)
        seen.append((seg.clone(), out))
        return out
    monkeypatch.setattr(tta_mod, "_postprocess_prediction", spy)
    data = iter([{"data": _synthetic_case(1), "data_properties": {}, "ofile": "tta_outputTs/case1"}]), 1
    bundle = (NS(), [16, 16, 16], net, [{k: v.clone() for k, v in net.state_dict().items()}])
    torch.manual_seed(0)
    np.random.seed(0)
    res = tta_mod.tta_main("run0", cfg, tmp_path, tmp_path, mapping, NS(ModifierFunctions=ModifierFunctions), "cuda:0",
                           network_bundle=bundle, tta_data=data)
    assert len(seen) == 1
    unfiltered = seen[0][0].numpy()
    want = R.filter_map(unfiltered, R.own_groups(3), 26)[0]
    written = np.load(res[("tta_outputTs/case1", "prediction")])
    assert written.shape == unfiltered.shape and np.array_equal(written, want)
    summary = json.loads((tmp_path / "run0" / "summary_Ts.json").read_text())
    for lab in (1, 2, 3):
        assert summary["metric_per_case"][0]["metrics"][str(lab)]["n_pred"] == int((want == lab).sum())


def test_a_stray_island_ruins_hd_and_the_filter_repairs_it():
    from dg_tta_amd.tta.evaluation import case_metrics
    from dg_tta_amd.tta.postprocessing import keep_largest_components
    ref, pred, noisy = _noisy_prediction()
    labels = [0, 1, 2, 3]
    clean = case_metrics(pred, ref, labels, DEV, surface=True)
    dirty = case_metrics(noisy, ref, labels, DEV, surface=True)
    island = np.sqrt(((np.argwhere(ref == 1) - np.array([10, 0, 0])) ** 2).sum(1).min())
    assert island > 5 and dirty[1]["HD"] >= island * (1 - 1e-6) and dirty[1]["HD"] > clean[1]["HD"]
    filtered, removed = keep_largest_components(noisy, [1])
    assert removed == {1: 1}
    repaired = case_metrics(filtered, ref, labels, DEV, surface=True)
    assert repaired[1] == clean[1]
