"""Code-sets query step, host side (no GPU): the C ABI declares and exports sylph_fcos_head_codesets / sylph_decode_nms_codesets, the
Engine-independent checks of a code-set list (offsets, validation messages), `class_code` together with `class_code_sets` is an error,
inference_on_dataset_with_code_sets shows evaluator g what the per-set loop shows it, and _do_test_meta_learning(fuse_repeats=True)
returns the results dict of the default loop."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "sylph_hip.h")) as f:
        return f.read()


def test_header_declares_the_two_entries():
    text = _header()
    m = re.search(r"int\s+sylph_fcos_head_codesets\s*\(([^;]*)\)\s*;", text)
    assert m, "include/sylph_hip.h does not declare sylph_fcos_head_codesets"
    assert len(m.group(1).split(",")) == 5
    m = re.search(r"int\s+sylph_decode_nms_codesets\s*\(([^;]*)\)\s*;", text)
    assert m, "include/sylph_hip.h does not declare sylph_decode_nms_codesets"
    assert len(m.group(1).split(",")) == 13
    for ref in ("fcos.py:582-667", "head_utils.py:60-81", "meta_learn_evaluation.py:421-426", "meta_fcos_runner.py:451-672"):
        assert ref in text


def test_library_exports_the_two_symbols():
    from sylph_amd import _lib
    assert len(_lib.PROTOTYPES["sylph_fcos_head_codesets"][1]) == 5
    assert len(_lib.PROTOTYPES["sylph_decode_nms_codesets"][1]) == 13
    L = _lib.lib()
    assert hasattr(L, "sylph_fcos_head_codesets") and hasattr(L, "sylph_decode_nms_codesets")


def test_code_set_offsets():
    from sylph_amd.engine import code_set_offsets
    assert code_set_offsets([5, 5, 1, 20]) == [0, 5, 10, 11, 31]
    assert code_set_offsets([32]) == [0, 32]
    with pytest.raises(ValueError, match="code set 1 is empty"):
        code_set_offsets([5, 0])


def test_check_code_sets_messages():
    from sylph_amd.engine import check_code_sets
    w5, b5 = torch.zeros(5, 256, 1, 1), torch.zeros(5)
    assert check_code_sets([(w5, b5), (torch.zeros(20, 256, 1, 1), torch.zeros(20))]) == [5, 20]
    assert check_code_sets([(torch.zeros(3, 512, 1, 1), None)]) == [3]  # (two CondConvBlock chunks: the engine refuses them on a CodeGenerator model)
    with pytest.raises(ValueError, match="at least one code set"):
        check_code_sets([])
    with pytest.raises(ValueError, match="code set 1 is empty"):
        check_code_sets([(w5, b5), (w5[:0], b5[:0])])
    with pytest.raises(ValueError, match="256 channels"):
        check_code_sets([(torch.zeros(5, 100, 1, 1), b5)])
    with pytest.raises(ValueError, match="dimension"):
        check_code_sets([(torch.zeros(5, 256), b5)])
    with pytest.raises(ValueError, match="spatial size 3x3"):
        check_code_sets([(torch.zeros(5, 256, 3, 3), b5)])
    with pytest.raises(ValueError, match="4 biases for 5 classes"):
        check_code_sets([(w5, torch.zeros(4))])
    with pytest.raises(ValueError, match="every code set or for none"):
        check_code_sets([(w5, b5), (w5, None)])
    with pytest.raises(NotImplementedError, match="CLS_LAYER"):
        check_code_sets([(w5, b5)], code_ksize=3)


def test_class_code_and_class_code_sets_exclude_each_other():
    from sylph_amd.modeling import check_class_code_args
    d = {"cls_conv": torch.zeros(5, 256, 1, 1), "cls_bias": torch.zeros(5)}
    assert check_class_code_args(d, None) is None and check_class_code_args(None, None) is None
    assert check_class_code_args(None, (d, d)) == [d, d]
    with pytest.raises(ValueError, match="both"):
        check_class_code_args(d, [d])
    with pytest.raises(ValueError, match="non-empty"):
        check_class_code_args(None, [])
    with pytest.raises(ValueError, match="non-empty"):
        check_class_code_args(None, d)
    with pytest.raises(ValueError, match=r"class_code_sets\[1\]"):
        check_class_code_args(None, [d, {"cls_bias": d["cls_bias"]}])


class _Model:
    """stands for the detector: a query image's "detection" is the first code value of the set it was scored with"""
    device = torch.device("cpu")

    def __init__(self):
        self.query_calls = 0

    def __call__(self, batched_inputs=None, class_code=None, run_type=None, class_code_sets=None):
        if run_type == "meta_learn_test_support":
            return {"cls_conv": torch.ones(1, 256, 1, 1) * float(batched_inputs[0]["seed"]), "cls_bias": torch.zeros(1, 1, 1, 1)}
        if run_type == "meta_learn_normalize_code":
            return class_code
        assert run_type == "meta_learn_test_instance"
        self.query_calls += 1
        one = lambda c: [{"seed_seen": None if c is None else float(c["cls_conv"][0, 0, 0, 0]), "image": x["image_id"]} for x in batched_inputs]
        if class_code_sets is not None:
            assert class_code is None
            return [one(c) for c in class_code_sets]
        return one(class_code)


class _Ev:
    def __init__(self):
        self.seen = []

    def reset(self):
        self.seen = []

    def process(self, inputs, outputs):
        assert len(inputs) == len(outputs)
        self.seen += [(x["image_id"], o["image"], o["seed_seen"]) for x, o in zip(inputs, outputs)]

    def evaluate(self):
        s = self.seen[0][2]
        ap = 40.0 if s is None else 10.0 + 2.0 * s
        return {"bbox": {"AP": ap, "AP50": 2 * ap, "APr": ap - 1}}


def test_inference_with_code_sets_shows_each_evaluator_its_own_set():
    from sylph_amd.evaluation import inference_on_dataset_with_class_codes, inference_on_dataset_with_code_sets
    loader = [[{"image_id": 0}, {"image_id": 1}], [{"image_id": 2}]]
    sets = [{"cls_conv": torch.full((3, 256, 1, 1), float(v))} for v in (1, 4, 7)]
    m, evs = _Model(), [_Ev() for _ in sets]
    res = inference_on_dataset_with_code_sets(m, loader, evs, sets)
    assert m.query_calls == len(loader)
    for g, c in enumerate(sets):
        ev = _Ev()
        want = inference_on_dataset_with_class_codes(_Model(), loader, ev, c)
        assert res[g] == want and evs[g].seen == ev.seen and len(ev.seen) == 3
    with pytest.raises(ValueError, match="one evaluator per set"):
        inference_on_dataset_with_code_sets(m, loader, evs[:2], sets)
    with pytest.raises(ValueError, match="empty"):
        inference_on_dataset_with_code_sets(m, loader, [], [])


def test_fuse_repeats_returns_the_unfused_results(tmp_path):
    from sylph_amd.runner import MetaFCOSRunner

    class Loader(list):
        pass

    class R(MetaFCOSRunner):
        def build_episodic_learning_detection_test_support_set_loader(self, cfg, name, seed=0):
            return Loader([[{"support_set": [], "support_set_target": torch.tensor(c), "class_name": str(c), "seed": seed}] for c in range(3)])

        def build_episodic_learning_detection_test_query_loader(self, cfg, name):
            return [[{"image_id": 0, "dataset": name}, {"image_id": 1, "dataset": name}], [{"image_id": 2, "dataset": name}]]

        def get_evaluator(self, cfg, name, output_folder=None):
            return _Ev()

    r = R()
    cfg = r.get_default_cfg()
    cfg.DATASETS.TEST = ("coco_meta_val_novel", "coco_meta_val_base")
    cfg.TEST.REPEAT_TEST = 3
    cfg.OUTPUT_DIR = str(tmp_path / "output")
    cfg.MODEL.META_LEARN.EVAL_WITH_PRETRAINED_CODE = True
    cfg.MODEL.META_LEARN.USE_ALL_GTS_IN_BASE_CLASSES = False
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    m0, m1 = _Model(), _Model()
    want = r._do_test_meta_learning(cfg, m0)
    got = r._do_test_meta_learning(cfg, m1, fuse_repeats=True)
    assert got == want and list(got) == ["default", "seed0", "seed1", "seed2"]
    assert [got[f"seed{s}"]["coco_meta_val_novel"]["bbox"]["AP"] for s in range(3)] == [10.0, 12.0, 14.0]
    top = got["default"]["coco_meta_val_novel"]["bbox"]
    assert abs(top["AP_avg"] - 12.0) < 1e-9 and abs(top["AP_std"] - np.std([10.0, 12.0, 14.0])) < 1e-9
    # two query batches per pass: novel 3 seeds + base (pretrained codes) 3 seeds unfused; novel once + base 3 times fused
    assert m0.query_calls == 2 * 6 and m1.query_calls == 2 * 4, (m0.query_calls, m1.query_calls)
    # REPEAT_TEST 1 (a non-final iteration): nothing to fuse, same dict
    assert r._do_test_meta_learning(cfg, _Model(), train_iter=10, fuse_repeats=True) == r._do_test_meta_learning(cfg, _Model(), train_iter=10)
