"""Mixed-episode query step, host side (no GPU): the C ABI declares and exports sylph_fcos_head_episodes, a list of class-code dicts is
grouped into episodes by identity, and a plain dict never reaches the new path."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sylph_hip.h")


def test_header_declares_and_library_exports_the_entry_point():
    from sylph_amd import _lib
    text = open(HEADER).read()
    m = re.search(r"int\s+sylph_fcos_head_episodes\s*\(([^;]*)\)\s*;", text)
    assert m, "include/sylph_hip.h does not declare sylph_fcos_head_episodes"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 6 and args[0].startswith("sylph_ctx*") and args[1].startswith("int ")
    assert all(a.startswith("const float*") for a in args[2:4]) and all(a.startswith("const int*") for a in args[4:6]), args
    assert "sylph_fcos_head_episodes" in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["sylph_fcos_head_episodes"][1]) == 6
    assert hasattr(_lib.lib(), "sylph_fcos_head_episodes")


def test_group_episodes_by_identity():
    from sylph_amd.modeling import group_episodes
    a, b, c = ({"cls_conv": torch.zeros(n, 256, 1, 1)} for n in (1, 2, 3))
    # interleaved: episodes in order of first appearance
    dicts, ie = group_episodes([b, a, b, c, a], 5)
    assert [id(d) for d in dicts] == [id(b), id(a), id(c)] and ie == [0, 1, 0, 2, 1]
    # repeated
    dicts, ie = group_episodes((a, a, b, b), 4)
    assert [id(d) for d in dicts] == [id(a), id(b)] and ie == [0, 0, 1, 1]
    # one episode for the whole batch
    dicts, ie = group_episodes([c, c, c], 3)
    assert len(dicts) == 1 and dicts[0] is c and ie == [0, 0, 0]
    # identity, not contents: an equal copy is another episode
    a2 = dict(a)
    dicts, ie = group_episodes([a, a2], 2)
    assert len(dicts) == 2 and ie == [0, 1]


def test_group_episodes_value_errors():
    from sylph_amd.modeling import group_episodes
    a = {"cls_conv": torch.zeros(1, 256, 1, 1)}
    with pytest.raises(ValueError, match="one class-code dict per input"):
        group_episodes([a, a], 3)
    with pytest.raises(ValueError, match="one class-code dict per input"):
        group_episodes([a, a, a], 2)
    with pytest.raises(ValueError, match="is None"):
        group_episodes([a, None], 2)


class _Head:
    """Stands in for MetaFCOS: records which entry the detector took."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _dets(n):
        z = torch.zeros
        return [{"pred_boxes": z(0, 4), "scores": z(0), "pred_classes": z(0, dtype=torch.long), "locations": z(0, 2),
                 "fpn_levels": z(0, dtype=torch.long)} for _ in range(n)]

    def __call__(self, w, b, out_sizes, raw=False):
        self.calls.append(("uniform", w, b))
        return self._dets(len(out_sizes))

    def forward_episodes(self, codes, image_episode, out_sizes):
        self.calls.append(("episodes", codes, image_episode))
        return self._dets(len(out_sizes))


def _detector(head):
    from sylph_amd.modeling import MetaOneStageDetector
    m = MetaOneStageDetector.__new__(MetaOneStageDetector)
    torch.nn.Module.__init__(m)
    m.eval()
    object.__setattr__(m, "proposal_generator", head)
    m.episodic_learning = True
    m._run_backbone = lambda batched_inputs: [(32, 48)] * len(batched_inputs)
    return m


def test_dict_keeps_the_uniform_path_and_list_takes_the_episodes_path():
    head = _Head()
    m = _detector(head)
    batch = [{"image": None}] * 4
    d0 = {"cls_conv": torch.zeros(5, 256, 1, 1), "cls_bias": torch.zeros(5)}
    d1 = {"cls_conv": torch.ones(3, 256, 1, 1), "cls_bias": torch.zeros(3), "cls_weight_norm": torch.ones(3)}
    out = m(batch, class_code=d0, run_type="meta_learn_test_instance")
    assert len(out) == 4 and [c[0] for c in head.calls] == ["uniform"]
    assert head.calls[0][1] is d0["cls_conv"] and head.calls[0][2] is d0["cls_bias"]
    head.calls.clear()
    out = m(batch, class_code=[d0, d1, d0, d1], run_type="meta_learn_test_instance")
    assert len(out) == 4 and [c[0] for c in head.calls] == ["episodes"]
    _, codes, ie = head.calls[0]
    assert ie == [0, 1, 0, 1] and len(codes) == 2
    assert codes[0][0] is d0["cls_conv"] and codes[0][1] is d0["cls_bias"] and codes[1][0] is d1["cls_conv"]
    head.calls.clear()
    with pytest.raises(ValueError):
        m(batch, class_code=[d0, d1], run_type="meta_learn_test_instance")
    with pytest.raises(ValueError):
        m(batch, class_code=[d0, None, d0, d1], run_type="meta_learn_test_instance")
    assert head.calls == []
