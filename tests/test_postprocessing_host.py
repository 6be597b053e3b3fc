"""CPU: the host logic of the connected-component post-processing (dg_tta_amd/tta/postprocessing.py): the plan keys, the group
specification, and the hook of run_tta that must not touch a prediction when no key asks for anything."""
import pytest
import torch

from dg_tta_amd.tta import postprocessing as pp
from dg_tta_amd.tta.config_log_utils import TEMPLATE_PLAN
from dg_tta_amd.tta.tta import _postprocess_prediction

LABELS = ["background", "liver", "spleen", "kidney_left", "kidney_right"]


def plan(**keys):
    return {"optimized_labels": LABELS, **keys}


def test_absent_and_false_ask_for_nothing():
    assert pp.postprocessing_groups(plan()) is None
    assert pp.postprocessing_groups(plan(postprocessing_keep_largest_component=False)) is None
    assert pp.postprocessing_settings(plan()) is None
    assert pp.postprocessing_settings(plan(postprocessing_keep_largest_component=False, postprocessing_min_component_voxels=0,
                                           postprocessing_connectivity=6)) is None
    assert not [k for k in TEMPLATE_PLAN if k.startswith("postprocessing")]           # prepare_tta writes what it wrote before


def test_true_foreground_names_indices_and_regions():
    assert pp.postprocessing_groups(plan(postprocessing_keep_largest_component=True)) == [1, 2, 3, 4]
    assert pp.postprocessing_groups(plan(postprocessing_keep_largest_component="foreground")) == "foreground"
    assert pp.postprocessing_groups(plan(postprocessing_keep_largest_component=["liver", 2])) == [1, 2]
    groups = pp.postprocessing_groups(plan(postprocessing_keep_largest_component=["spleen", ["kidney_left", 4], 1]))
    assert groups == [2, (3, 4), 1]             # a nested list (JSON has no tuples) is a region


def test_settings_carry_every_key():
    s = pp.postprocessing_settings(plan(postprocessing_keep_largest_component=True, postprocessing_min_component_voxels=10,
                                        postprocessing_connectivity=18))
    assert s == dict(labels_or_regions=[1, 2, 3, 4], connectivity=18, min_voxels=10, keep_largest=True)
    s = pp.postprocessing_settings(plan(postprocessing_min_component_voxels=3))         # the threshold alone: every label, no winner
    assert s == dict(labels_or_regions=[1, 2, 3, 4], connectivity=26, min_voxels=3, keep_largest=False)


def test_duplicates_say_to_call_twice():
    with pytest.raises(ValueError, match="call twice"):
        pp.postprocessing_groups(plan(postprocessing_keep_largest_component=["liver", ["liver", "spleen"]]))
    with pytest.raises(ValueError, match="call twice"):
        pp._entries([1, (2, 1)])
    with pytest.raises(ValueError, match="call twice"):
        pp._entries([(3, 3)])


def test_unknown_names_and_indices_are_named():
    with pytest.raises(ValueError, match="'pancreas'"):
        pp.postprocessing_groups(plan(postprocessing_keep_largest_component=["liver", "pancreas"]))
    with pytest.raises(ValueError, match="index 5"):
        pp.postprocessing_groups(plan(postprocessing_keep_largest_component=[5]))
    with pytest.raises(ValueError, match="index -1"):
        pp.postprocessing_groups(plan(postprocessing_keep_largest_component=[[1, -1]]))
    with pytest.raises(ValueError, match="index True"):
        pp.postprocessing_groups(plan(postprocessing_keep_largest_component=[True]))
    with pytest.raises(ValueError, match="'largest'"):
        pp.postprocessing_groups(plan(postprocessing_keep_largest_component="largest"))
    with pytest.raises(ValueError, match="1024"):
        pp._entries([1024])


@pytest.mark.parametrize("bad", [4, 8, 27, "26", None, True, 6.5])
def test_bad_connectivity(bad):
    with pytest.raises(ValueError, match="connectivity"):
        pp.postprocessing_settings(plan(postprocessing_keep_largest_component=True, postprocessing_connectivity=bad))
    with pytest.raises(ValueError, match="connectivity"):
        pp.postprocessing_settings(plan(postprocessing_connectivity=bad))             # a bad value is reported even when unused


@pytest.mark.parametrize("bad", [-1, 2.5, "3", True])
def test_bad_min_voxels(bad):
    with pytest.raises(ValueError, match="postprocessing_min_component_voxels"):
        pp.postprocessing_settings(plan(postprocessing_min_component_voxels=bad))


def test_hook_returns_the_same_object_when_nothing_is_asked_for():
    seg = torch.zeros((2, 3, 4), dtype=torch.int64)
    for cfg in (plan(), plan(postprocessing_keep_largest_component=False), plan(postprocessing_connectivity=18)):
        assert _postprocess_prediction(seg, cfg, "cuda") is seg                        # no copy, and no GPU on this machine


def test_nnunet_name_is_exported_with_its_argument_order():
    import inspect
    sig = inspect.signature(pp.remove_all_but_largest_component_from_segmentation)
    assert list(sig.parameters) == ["segmentation", "labels_or_regions", "background_label"]
    assert sig.parameters["background_label"].default == 0
    assert "UNPINNED" in pp.remove_all_but_largest_component_from_segmentation.__doc__
