"""CPU: the two pure functions under the detector's four `*train_step` entries
(pair-net_amd/detector.py: `unpack_batch`, `parse_losses`) and the runner's two tables, which are
views of `detector.TRAIN_ENTRIES` and must stay what they were when they were written out."""
import pytest
import torch

from pairnet_amd.detector import TRAIN_ENTRIES, parse_losses, unpack_batch


class _Container:
    """Stand-in for mmcv's DataContainer: the payload is `.data`."""

    def __init__(self, data):
        self.data = data


def _plain():
    return dict(img=torch.zeros(2, 3, 4, 6), img_metas=[dict(i=0), dict(i=1)],
                gt_rels=[torch.tensor([[0, 1, 5]]), torch.tensor([[1, 0, 2]])],
                gt_bboxes=[torch.zeros(2, 4), torch.ones(3, 4)],
                gt_labels=[torch.tensor([3, 7]), torch.tensor([1, 2, 4])],
                gt_masks=[torch.zeros(2, 4, 6), torch.ones(3, 4, 6)])


ORDER = ("img", "img_metas", "gt_rels", "gt_bboxes", "gt_labels", "gt_masks")


def _same(got, want):
    assert len(got) == len(ORDER)
    # (a bare tensor has a `.data` of its own, so `img` comes back as an alias of the same memory)
    assert got[0].data_ptr() == want["img"].data_ptr() and got[0].shape == want["img"].shape
    for g, k in zip(got[1:], ORDER[1:]):
        assert g is want[k], k


def test_unpack_batch_plain_values():
    d = _plain()
    _same(unpack_batch(d), d)
    _same(unpack_batch(d, need=("gt_bboxes",)), d)


def test_unpack_batch_data_containers():
    d = _plain()
    _same(unpack_batch({k: _Container(v) for k, v in d.items()}), d)


def test_unpack_batch_single_element_lists():
    d = _plain()
    wrapped = {k: ([v] if k != "img" else v) for k, v in d.items()}       # [[...]]
    _same(unpack_batch(wrapped), d)
    _same(unpack_batch({k: _Container(v) for k, v in wrapped.items()}), d)
    # a list of ONE tensor (a batch of one image) is no [[...]] form and stays a list
    one = dict(d, gt_labels=[d["gt_labels"][0]])
    assert unpack_batch(one)[4] is one["gt_labels"]


def test_unpack_batch_img_as_one_element_list():
    d = _plain()
    _same(unpack_batch(dict(d, img=[d["img"]])), d)
    _same(unpack_batch(dict(d, img=_Container((d["img"],)))), d)


def test_unpack_batch_missing_keys():
    d = _plain()
    for key, need in (("gt_masks", ("gt_masks",)), ("gt_bboxes", ("gt_bboxes",))):
        less = {k: v for k, v in d.items() if k != key}
        with pytest.raises(KeyError):
            unpack_batch(less, need=need)
    for key in ("img", "img_metas", "gt_rels", "gt_labels"):
        with pytest.raises(KeyError):
            unpack_batch({k: v for k, v in d.items() if k != key})
    # what the entry does not need may be missing: it comes back as None
    got = unpack_batch({k: v for k, v in d.items() if k != "gt_bboxes"})
    assert got[3] is None and got[5] is d["gt_masks"]
    got = unpack_batch({k: v for k, v in d.items() if k != "gt_masks"}, need=("gt_bboxes",))
    assert got[5] is None and got[3] is d["gt_bboxes"]


def test_parse_losses():
    out = {"loss_cls": torch.tensor(0.5), "d0.loss_mask": torch.tensor(0.25),
           "r_loss_cls": torch.tensor(2.0), "grad_norm": torch.tensor(64.0),
           "assign_status": torch.tensor(3, dtype=torch.int32)}
    got = parse_losses(out, 2)
    assert set(got) == {"loss", "log_vars", "num_samples"} and got["num_samples"] == 2
    assert isinstance(got["loss"], torch.Tensor) and float(got["loss"]) == 0.5 + 0.25 + 2.0
    assert got["log_vars"] == {"loss_cls": 0.5, "d0.loss_mask": 0.25, "r_loss_cls": 2.0,
                               "grad_norm": 64.0, "assign_status": 3.0, "loss": 2.75}
    assert all(type(v) is float for v in got["log_vars"].values())
    assert list(got["log_vars"]) == list(out) + ["loss"]


def test_runner_tables_are_the_parent_commits():
    from pairnet_amd import runner
    assert runner.ENTRIES == {
        "TailTrainer": ("train_step", "_trainer", "trainer"),
        "BaselineTrainer": ("full_train_step", "_full_trainer", "full_trainer"),
        "BBoxTrainer": ("box_train_step", "_box_trainer", "box_trainer"),
        "PSGTr2Trainer": ("triplet_train_step", "_triplet_trainer", "triplet_trainer")}
    assert runner.HEAD_TRAINER == {"CrossHead2": "TailTrainer", "CrossHeadBaseline": "BaselineTrainer",
                                   "CrossHeadBBox": "BBoxTrainer", "PSGTrHead2": "PSGTr2Trainer"}
    assert list(runner.ENTRIES) == list(TRAIN_ENTRIES)
    # the one field the tables do not show: only the box entry takes no ground-truth masks
    assert {n: r.masks for n, r in TRAIN_ENTRIES.items()} == {
        "TailTrainer": True, "BaselineTrainer": True, "BBoxTrainer": False, "PSGTr2Trainer": True}
    import pairnet_amd as P
    for name, row in TRAIN_ENTRIES.items():
        assert hasattr(P, name) and hasattr(P, row.head)
        assert callable(getattr(P.PSGTr, row.step)) and callable(getattr(P.PSGTr, row.builder))
