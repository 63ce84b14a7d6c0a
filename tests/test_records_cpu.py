"""Query records, host side (no GPU): the C ABI declares and binds the record entries, cache_query_dataset makes one model call per
batch and keeps no image tensors, the evaluation loops over records show the evaluators the original metadata in loader order, the
max_bytes refusal fires before the store that would pass it, and _do_test_meta_learning(cache_queries=True) returns the results dict of
the plain loop at one network pass per dataset."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"sylph_fcos_towers": 1, "sylph_record_store": 2, "sylph_record_load": 2, "sylph_record_info": 5, "sylph_record_destroy": 2}


def test_header_declares_and_lib_binds_every_record_entry():
    from sylph_amd import _lib
    with open(os.path.join(ROOT, "include", "sylph_hip.h")) as f:
        text = f.read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"(?:int|void)\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"include/sylph_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs, name
        assert len(_lib.PROTOTYPES[name][1]) == nargs, name
    for ref in ("fcos.py:582-667", "meta_learn_evaluation.py:367-470", "meta_fcos_runner.py:451-672"):
        assert ref in text[text.index("Query records"):]
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name


class _Record:
    """stands for a QueryRecord: remembers whether it was closed"""

    def __init__(self, n, nbytes):
        self.batch = (n, 128, 160, [(128, 160)] * n)
        self.nbytes = nbytes
        self.closed = False

    def close(self):
        self.closed = True


class _Model:
    """stands for the detector: a query image's "detection" is the first code value of the set it was scored with; a cache-query call keeps
    the inputs' metadata and a _Record; `network_passes` counts the calls that would run the backbone and the towers"""
    device = torch.device("cpu")
    META = ("image_id", "file_name", "height", "width")

    def __init__(self, bytes_per_image=100):
        self.network_passes, self.record_scores, self.calls, self.records = 0, 0, [], []
        self.bytes_per_image = bytes_per_image

    def __call__(self, batched_inputs=None, class_code=None, run_type=None, class_code_sets=None):
        if run_type == "meta_learn_test_support":
            return {"cls_conv": torch.ones(1, 256, 1, 1) * float(batched_inputs[0]["seed"]), "cls_bias": torch.zeros(1, 1, 1, 1)}
        if run_type == "meta_learn_normalize_code":
            return class_code
        self.calls.append((run_type, [x.get("image_id") for x in batched_inputs]))
        if run_type == "meta_learn_cache_query":
            self.network_passes += 1
            rec = _Record(len(batched_inputs), self.bytes_per_image * len(batched_inputs))
            self.records.append(rec)
            return [{"record": rec, "inputs": [{k: x[k] for k in self.META if k in x} for x in batched_inputs]}]
        assert run_type == "meta_learn_test_instance"
        if len(batched_inputs) == 1 and "record" in batched_inputs[0]:
            assert not batched_inputs[0]["record"].closed
            self.record_scores += 1
            batched_inputs = batched_inputs[0]["inputs"]
        else:
            self.network_passes += 1
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
        assert all("image" not in x and "record" not in x for x in inputs) or all("image" in x for x in inputs)
        self.seen += [(x["image_id"], x.get("file_name"), x.get("height"), o["image"], o["seed_seen"]) for x, o in zip(inputs, outputs)]

    def evaluate(self):
        s = self.seen[0][4]
        ap = 40.0 if s is None else 10.0 + 2.0 * s
        return {"bbox": {"AP": ap, "AP50": 2 * ap, "APr": ap - 1}}


def _loader():
    im = lambda: torch.zeros(3, 8, 8)
    return [[{"image": im(), "image_id": 0, "file_name": "a.jpg", "height": 480, "width": 640},
             {"image": im(), "image_id": 1, "file_name": "b.jpg", "height": 300, "width": 400}],
            [{"image": im(), "image_id": 2, "file_name": "c.jpg", "height": 200, "width": 100}],
            [{"image": im(), "image_id": 3, "file_name": "d.jpg", "height": 64, "width": 96},
             {"image": im(), "image_id": 4, "file_name": "e.jpg", "height": 128, "width": 160}]]


def _tensors(obj):
    if torch.is_tensor(obj):
        return 1
    if isinstance(obj, dict):
        return sum(_tensors(v) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return sum(_tensors(v) for v in obj)
    return 0


def test_cache_query_dataset_one_call_per_batch_and_no_image_tensors():
    from sylph_amd.evaluation import cache_query_dataset, release_query_records
    m, loader = _Model(), _loader()
    recs = cache_query_dataset(m, loader, max_bytes=10 ** 6)
    assert m.calls == [("meta_learn_cache_query", [0, 1]), ("meta_learn_cache_query", [2]), ("meta_learn_cache_query", [3, 4])]
    assert len(recs) == len(loader) and all(len(item) == 1 for item in recs)
    assert _tensors(recs) == 0, "the record list keeps image tensors"
    assert [[x["image_id"] for x in item[0]["inputs"]] for item in recs] == [[0, 1], [2], [3, 4]]
    assert recs[1][0]["inputs"][0] == {"image_id": 2, "file_name": "c.jpg", "height": 200, "width": 100}
    release_query_records(recs)
    assert all(r.closed for r in m.records)


def test_evaluation_loops_over_records_show_the_original_metadata():
    from sylph_amd.evaluation import cache_query_dataset, inference_on_dataset_with_class_codes, inference_on_dataset_with_code_sets
    loader = _loader()
    sets = [{"cls_conv": torch.full((3, 256, 1, 1), float(v))} for v in (1, 4, 7)]
    m = _Model()
    recs = cache_query_dataset(m, loader, max_bytes=10 ** 6)
    assert m.network_passes == len(loader)
    for c in sets:
        ev, ev_plain = _Ev(), _Ev()
        got = inference_on_dataset_with_class_codes(m, recs, ev, c)
        want = inference_on_dataset_with_class_codes(_Model(), loader, ev_plain, c)
        assert got == want and ev.seen == ev_plain.seen and [s[0] for s in ev.seen] == [0, 1, 2, 3, 4]
        assert ev.seen[2][1:3] == ("c.jpg", 200)
    evs, evs_plain = [_Ev() for _ in sets], [_Ev() for _ in sets]
    got = inference_on_dataset_with_code_sets(m, recs, evs, sets)
    want = inference_on_dataset_with_code_sets(_Model(), loader, evs_plain, sets)
    assert got == want and [e.seen for e in evs] == [e.seen for e in evs_plain]
    assert m.network_passes == len(loader) and m.record_scores == 4 * len(loader)  # every later call scored a record


def test_max_bytes_refusal_fires_before_the_offending_store():
    from sylph_amd.evaluation import cache_query_dataset
    # the loader's length is known: the first record (200 bytes) shows that three batches will not fit 450 bytes
    m = _Model()
    with pytest.raises(MemoryError, match=r"needs 600 bytes.* 450 are allowed"):
        cache_query_dataset(m, _loader(), max_bytes=450)
    assert m.network_passes == 1 and all(r.closed for r in m.records)
    # no length: batch by batch at the bytes per image seen so far -- 200 + 100 fit 450, the third batch (200 more) is never run
    m = _Model()
    with pytest.raises(MemoryError, match=r"needs 500 bytes.* 450 are allowed"):
        cache_query_dataset(m, iter(_loader()), max_bytes=450)
    assert [c[1] for c in m.calls] == [[0, 1], [2]] and all(r.closed for r in m.records)
    # a limit that fits: nothing is refused
    m = _Model()
    assert len(cache_query_dataset(m, _loader(), max_bytes=600)) == 3 and not any(r.closed for r in m.records)


def test_cache_queries_returns_the_plain_results_at_one_pass_per_dataset(tmp_path, caplog):
    from sylph_amd.runner import MetaFCOSRunner

    class Loader(list):
        pass

    class R(MetaFCOSRunner):
        def build_episodic_learning_detection_test_support_set_loader(self, cfg, name, seed=0):
            return Loader([[{"support_set": [], "support_set_target": torch.tensor(c), "class_name": str(c), "seed": seed}] for c in range(3)])

        def build_episodic_learning_detection_test_query_loader(self, cfg, name):
            return [[dict(x, dataset=name) for x in item] for item in _loader()]

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
    got = r._do_test_meta_learning(cfg, m1, cache_queries=True, cache_max_bytes=10 ** 6)
    assert got == want and list(got) == ["default", "seed0", "seed1", "seed2"]
    assert [got[f"seed{s}"]["coco_meta_val_novel"]["bbox"]["AP"] for s in range(3)] == [10.0, 12.0, 14.0]
    # three query batches per pass: 2 datasets x 3 seeds plain; one pass per dataset cached, and 2 x 3 x 3 record scores
    assert m0.network_passes == 3 * 6 and m0.record_scores == 0
    assert m1.network_passes == 3 * 2 and m1.record_scores == 3 * 6
    assert all(rec.closed for rec in m1.records), "the runner leaves query records allocated"
    # a budget the first record already shows to be too small: the plain loop, with a logged reason, the same dict
    m2 = _Model()
    with caplog.at_level("INFO", logger="sylph_amd.runner"):
        assert r._do_test_meta_learning(cfg, m2, cache_queries=True, cache_max_bytes=450) == want
    assert "keeps one network pass per seed" in caplog.text and "450 are allowed" in caplog.text
    assert m2.record_scores == 0 and m2.network_passes == 3 * 6 + 2 and all(rec.closed for rec in m2.records)
    # off by default, and with fuse_repeats the fused datasets need no records
    m3 = _Model()
    assert r._do_test_meta_learning(cfg, m3, fuse_repeats=True, cache_queries=True, cache_max_bytes=10 ** 6) == want
    assert m3.network_passes == 3 + 3 and m3.record_scores == 3 * 3  # novel: one fused pass; base (pretrained codes): one pass, three scores
