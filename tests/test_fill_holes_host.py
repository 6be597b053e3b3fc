"""CPU: the host logic of the hole filling (dg_tta_amd/tta/postprocessing.py): the plan keys `postprocessing_fill_holes` and
`postprocessing_fill_holes_connectivity`, their errors, and the hook of run_tta that must not touch a prediction - nor the GPU -
when no key asks for anything."""
import inspect

import pytest
import torch

from dg_tta_amd.tta import postprocessing as pp
from dg_tta_amd.tta.config_log_utils import TEMPLATE_PLAN
from dg_tta_amd.tta.tta import _postprocess_prediction

LABELS = ["background", "liver", "spleen", "kidney_left", "kidney_right"]


def plan(**keys):
    return {"optimized_labels": LABELS, **keys}


def test_absent_and_false_ask_for_nothing():
    assert pp.fill_holes_settings(plan()) is None
    assert pp.fill_holes_settings(plan(postprocessing_fill_holes=False)) is None
    assert pp.fill_holes_settings(plan(postprocessing_fill_holes=None, postprocessing_fill_holes_connectivity=26)) is None
    assert pp.fill_holes_settings(plan(postprocessing_keep_largest_component=True)) is None       # the other key is another matter
    assert not [k for k in TEMPLATE_PLAN if k.startswith("postprocessing")]                         # prepare_tta writes what it wrote before


def test_true_names_indices_and_regions():
    assert pp.fill_holes_settings(plan(postprocessing_fill_holes=True)) == dict(labels_or_regions=[1, 2, 3, 4], connectivity=6)
    s = pp.fill_holes_settings(plan(postprocessing_fill_holes=["spleen", ["kidney_left", 4], 1], postprocessing_fill_holes_connectivity=18))
    assert s == dict(labels_or_regions=[2, (3, 4), 1], connectivity=18)     # listed order is processing order; a nested list is a region
    assert pp.fill_holes_settings(plan(postprocessing_fill_holes=["liver"], postprocessing_connectivity=18))["connectivity"] == 6


def test_foreground_names_no_fill_label():
    with pytest.raises(ValueError, match="postprocessing_fill_holes: 'foreground'"):
        pp.fill_holes_settings(plan(postprocessing_fill_holes="foreground"))
    assert pp.postprocessing_groups(plan(postprocessing_keep_largest_component="foreground")) == "foreground"   # that key still takes it


def test_duplicates_unknown_names_and_indices_are_named_with_the_key():
    with pytest.raises(ValueError, match="call twice"):
        pp.fill_holes_settings(plan(postprocessing_fill_holes=["liver", ["liver", "spleen"]]))
    with pytest.raises(ValueError, match="postprocessing_fill_holes: label name 'pancreas'"):
        pp.fill_holes_settings(plan(postprocessing_fill_holes=["liver", "pancreas"]))
    with pytest.raises(ValueError, match="postprocessing_fill_holes: label index 5"):
        pp.fill_holes_settings(plan(postprocessing_fill_holes=[5]))
    with pytest.raises(ValueError, match="index -1"):
        pp.fill_holes_settings(plan(postprocessing_fill_holes=[[1, -1]]))
    with pytest.raises(ValueError, match="index True"):
        pp.fill_holes_settings(plan(postprocessing_fill_holes=[True]))
    with pytest.raises(ValueError, match="'all'"):
        pp.fill_holes_settings(plan(postprocessing_fill_holes="all"))
    with pytest.raises(ValueError, match="postprocessing_fill_holes: 3"):
        pp.fill_holes_settings(plan(postprocessing_fill_holes=3))


@pytest.mark.parametrize("bad", [4, 8, 27, "6", None, True, 6.5])
def test_bad_connectivity(bad):
    with pytest.raises(ValueError, match="connectivity"):
        pp.fill_holes_settings(plan(postprocessing_fill_holes=True, postprocessing_fill_holes_connectivity=bad))
    with pytest.raises(ValueError, match="connectivity"):
        pp.fill_holes_settings(plan(postprocessing_fill_holes_connectivity=bad))      # a bad value is reported even when unused


def test_hook_returns_the_same_object_when_nothing_is_asked_for():
    seg = torch.zeros((2, 3, 4), dtype=torch.int64)
    for cfg in (plan(), plan(postprocessing_fill_holes=False), plan(postprocessing_fill_holes_connectivity=18)):
        assert _postprocess_prediction(seg, cfg, "cuda") is seg                        # no copy, and no GPU on this machine


def test_function_signatures_and_the_unpinned_mark():
    sig = inspect.signature(pp.fill_label_holes)
    assert list(sig.parameters) == ["label_map", "labels_or_regions", "connectivity", "background", "device"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [None, 6, 0, "cuda"]
    assert "UNPINNED" in pp.fill_label_holes.__doc__
    from dg_tta_amd.tta import preprocessing
    assert list(inspect.signature(preprocessing.crop_to_nonzero_gpu).parameters) == ["data", "seg", "device", "nonzero_label"]
    with pytest.raises(ValueError, match="foreground"):
        pp.fill_label_holes(torch.zeros((2, 3, 4), dtype=torch.int64), "foreground", device="cpu")
