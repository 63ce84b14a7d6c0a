"""Class-code fine-tuning on the GPU (csrc/finetune.hip through Engine.fcos_targets / Engine.cls_grad / sylph_amd.finetune), on the synthetic
head over imported pyramids.

Yardsticks: tests/finetune_ref.py.  The targets are compared exactly (the restatement is pinned to the reference by
tests/golden/g12_fcos_targets.npz).  Loss and gradients are compared with the float64 restatement on the operand values the kernel
feeds its MFMAs (the `export_tower` taps of the same batch, normalised by oracle.bf16.gn_apply; codes rounded to bf16; g as bf16 hi + lo):
per output element |err| <= n_rows * 2^-23 * A, A the float64 sum of the absolute terms of that element -- the worst case of an fp32 chain
of n_rows adds, doubled for the exp / pow intrinsics.  Everything else is bit equality between two runs of the library."""
import math
import os

import numpy as np
import pytest
import torch

import finetune_ref as FR
from test_hip_parity import _cfg, _roienc_cfg

pytestmark = pytest.mark.gpu
HW = (128, 160)
SIZES = [(128, 153), (123, 160)]
ROWS = 2 * 428


def _sd(**kw):
    from sylph_amd import synthetic as W
    return W.head_state_dict(seed=3, **kw)


def _engine(dtype="bf16", cfg=None, sd=None, taps=True):
    from sylph_amd.engine import Engine
    eng = Engine(cfg if cfg is not None else _cfg(), dtype=dtype)
    eng.load_state_dict(sd if sd is not None else _sd())
    if taps:
        eng.set_debug_taps(True)
    return eng


def _codes(n, seed, scale=2.5):
    from sylph_amd import synthetic as W
    c = W.synthetic_codes(n, seed=seed, scale=scale)
    return c["cls_conv"].cuda(), c["cls_bias"].cuda()


def _operand(eng):
    """the normalised last cls tower layer of the current fresh batch as the kernels read it: (rows, 256) on the host"""
    from oracle import bf16 as OB16
    ys, cfs = eng.export_tower(0, 3)
    return FR.rows_of([OB16.gn_apply(y.cpu(), cf.cpu()) for y, cf in zip(ys, cfs)])


@pytest.fixture(scope="module")
def small():
    """one engine, the two-image ragged 128 x 160 batch: its pyramid, its operand values and its record"""
    eng = _engine()
    feats = FR.pyramid(2, HW, seed=7)
    eng.import_pyramid(feats, HW, SIZES)
    eng.towers()
    xn = _operand(eng)
    assert xn.shape == (ROWS, 256)
    rec = eng.store_record()
    yield {"eng": eng, "feats": feats, "xn": xn, "rec": rec}
    eng.close()


def _labels(n, seed=5):
    """labels of the small batch for n classes: a tenth of image 0's rows positive; class 1 (n >= 5) has no positive, image 1 has none"""
    g = torch.Generator().manual_seed(seed + n)
    lab = torch.full((ROWS,), -1, dtype=torch.int32)
    pos = torch.rand(428, generator=g) < 0.1
    cls = torch.randint(0, n, (428,), generator=g, dtype=torch.int32)
    if n >= 5:
        cls[cls == 1] = 0
    lab[:428][pos] = cls[pos]
    assert (lab[428:] == -1).all() and (lab >= 0).any()
    return lab


# ------------------------------------------------------------------------------------------------ 1: targets
@pytest.mark.parametrize("case", ["a_on", "a_off", "b_on", "c_on", "d_on"])
def test_targets_golden_batch_on_a_record(small, golden_dir, case):
    g = np.load(os.path.join(golden_dir, "g12_fcos_targets.npz"))
    eng = small["eng"]
    eng.load_record(small["rec"])
    cs = bool(g[f"{case}_center_sample"])
    keep = eng.fcos_train["center_sample"]
    eng.fcos_train["center_sample"] = cs
    try:
        labels, npos = eng.fcos_targets(torch.from_numpy(g[f"{case}_boxes"]), torch.from_numpy(g[f"{case}_classes"]),
                                        torch.from_numpy(g[f"{case}_image"]))
    finally:
        eng.fcos_train["center_sample"] = keep
    want = FR.fcos_targets_ref(g[f"{case}_boxes"], g[f"{case}_classes"], g[f"{case}_image"], 2, FR.levels(HW), center_sample=cs)
    assert np.array_equal(labels.cpu().numpy(), want), f"{case}: {int((labels.cpu().numpy() != want).sum())} labels differ"
    assert int(npos) == int((want >= 0).sum()) > 0


def test_targets_random_boxes_three_images():
    hw = (256, 320)
    eng = _engine(taps=False)
    eng.import_pyramid(FR.pyramid(3, hw, seed=8), hw)
    eng.towers()
    ann = FR.random_boxes(3, 40, hw, 20, seed=9, lo=4.0, hi=300.0)
    for cs in (True, False):
        eng.fcos_train["center_sample"] = cs
        labels, npos = eng.fcos_targets(ann["boxes"], ann["classes"], ann["image_index"])
        want = FR.fcos_targets_ref(ann["boxes"].numpy(), ann["classes"].numpy(), ann["image_index"].numpy(), 3, FR.levels(hw), center_sample=cs)
        assert labels.numel() == 3 * 1706 and np.array_equal(labels.cpu().numpy(), want)
        assert int(npos) == int((want >= 0).sum()) > 100
    eng.close()


# ------------------------------------------------------------------------------------------------ 2: loss, gradient, bias gradient
@pytest.mark.parametrize("n", [1, 5, 32, 33, 60])
def test_gradient_against_restatement(small, n):
    eng = small["eng"]
    eng.load_record(small["rec"])
    w, b = _codes(n, seed=40 + n)
    lab = _labels(n)
    loss, gw, gb = eng.cls_grad(lab.cuda(), w, b)
    fc = eng.fcos_train
    ref = FR.cls_grad_ref(small["xn"], lab, w.cpu().reshape(n, 256), b.cpu(), fc["alpha"], fc["gamma"])
    bound = ROWS * 2.0 ** -23
    worst = {}
    for name, got, want, A in (("loss", loss.cpu().double().reshape(()), ref["loss"], ref["A_loss"]),
                               ("grad_w", gw.cpu().double(), ref["gw"], ref["A_gw"]), ("grad_b", gb.cpu().double(), ref["gb"], ref["A_gb"])):
        assert got.shape == want.shape
        ratio = ((got - want).abs() / (bound * A).clamp(min=1e-300)).max()
        worst[name] = float(ratio)
    print(f"N = {n}: worst |err| / (n_rows 2^-23 A): {worst}")
    assert float(ref["A_gw"].min()) > 0 and float(ref["gw"].abs().max()) > 1e-3, "the comparison proves nothing"
    for name, r in worst.items():
        assert r <= 1.0, f"N = {n}: {name} misses its bound by a factor {r:.3g}"


def test_gradient_many_units_and_any_grid(monkeypatch):
    """40 images: 280 tiles = 70 units of 16 row groups, more than the 64 one reduce pass sums, so cls_grad_sum_kernel runs; and the same
    call under a block cap of 1 and of 3 (a wave takes 18 resp. 6 units) gives the same bits"""
    eng = _engine()
    eng.import_pyramid(FR.pyramid(40, HW, seed=12), HW)
    eng.towers()
    xn = _operand(eng)
    rows = 40 * 428
    g = torch.Generator().manual_seed(13)
    lab = torch.where(torch.rand(rows, generator=g) < 0.05, torch.randint(0, 5, (rows,), generator=g), torch.tensor(-1)).to(torch.int32)
    w, b = _codes(5, seed=105)
    loss, gw, gb = eng.cls_grad(lab.cuda(), w, b)
    fc = eng.fcos_train
    ref = FR.cls_grad_ref(xn, lab, w.cpu().reshape(5, 256), b.cpu(), fc["alpha"], fc["gamma"])
    bound = rows * 2.0 ** -23
    for name, got, want, A in (("loss", loss.cpu().double().reshape(()), ref["loss"], ref["A_loss"]),
                               ("grad_w", gw.cpu().double(), ref["gw"], ref["A_gw"]), ("grad_b", gb.cpu().double(), ref["gb"], ref["A_gb"])):
        r = float(((got - want).abs() / (bound * A)).max())
        print(f"70 units: {name}: worst |err| / (n_rows 2^-23 A) = {r:.4g}")
        assert r <= 1.0, f"{name} misses its bound by a factor {r:.3g}"
    for cap in ("1", "3"):
        monkeypatch.setenv("SYLPH_CLS_GRAD_BLOCKS", cap)
        l2, gw2, gb2 = eng.cls_grad(lab.cuda(), w, b)
        assert torch.equal(l2, loss) and torch.equal(gw2, gw) and torch.equal(gb2, gb), f"block cap {cap}: other bits"
    monkeypatch.delenv("SYLPH_CLS_GRAD_BLOCKS")
    eng.close()


# ------------------------------------------------------------------------------------------------ 3: class_offset blocks
def test_class_offset_blocks_are_bit_identical(small):
    eng = small["eng"]
    eng.load_record(small["rec"])
    w, b = _codes(60, seed=100)
    lab = _labels(60).cuda()
    loss, gw, gb = eng.cls_grad(lab, w, b)
    la, gwa, gba = eng.cls_grad(lab, w[:32], b[:32], check_labels=False)
    lb, gwb, gbb = eng.cls_grad(lab, w[32:], b[32:], class_offset=32)
    assert torch.equal(gw, torch.cat([gwa, gwb])) and torch.equal(gb, torch.cat([gba, gbb]))
    assert torch.equal(loss, la + lb)
    assert float(gwb.abs().max()) > 0 and float(gwa.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 4: reproducible bits
def test_same_bits_twice_and_fresh_against_record(small):
    eng = small["eng"]
    w, b = _codes(33, seed=101)
    lab = _labels(33).cuda()
    eng.load_record(small["rec"])
    first = eng.cls_grad(lab, w, b)
    again = eng.cls_grad(lab, w, b)
    eng.import_pyramid(small["feats"], HW, SIZES)
    eng.towers()
    fresh = eng.cls_grad(lab, w, b)
    for other in (again, fresh):
        for x, y in zip(first, other):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 5: non-interference
def test_head_and_decode_do_not_see_the_gradient_calls(small, golden_dir):
    eng = small["eng"]
    g = np.load(os.path.join(golden_dir, "g12_fcos_targets.npz"))
    w, b = _codes(5, seed=102, scale=3.0)

    def run(between):
        eng.load_record(small["rec"])
        if between in ("before", "both"):
            labels, _ = eng.fcos_targets(torch.from_numpy(g["a_on_boxes"]), torch.from_numpy(g["a_on_classes"]), torch.from_numpy(g["a_on_image"]))
            eng.cls_grad(labels, w, b)
        eng.head(w, b)
        if between == "both":
            eng.cls_grad(_labels(5).cuda(), w, b)
        return eng.decode(), eng.export_head()
    want_d, want_h = run(None)
    assert all(d["scores"].numel() > 0 for d in want_d), "no detection: the comparison proves nothing"
    for between in ("before", "both"):
        got_d, got_h = run(between)
        for x, y in zip(got_d, want_d):
            for k in ("pred_boxes", "scores", "pred_classes", "fpn_levels", "locations", "cand_index"):
                assert torch.equal(x[k], y[k]), f"{between}: {k} differs"
        for xs, ys in zip(got_h, want_h):
            for x, y in zip(xs, ys):
                assert torch.equal(x, y), f"{between}: an exported head tensor differs"


# ------------------------------------------------------------------------------------------------ 6: the loop
def test_loop_halves_the_loss_and_keeps_frozen_rows():
    """finetune_class_codes on four records from zero codes with the prior bias, lr 0.05, momentum 0.9, weight decay 1e-4, 200 steps.  lr was
    chosen on the CPU: the float64 restatement alone (finetune_ref.loop_ref on the oracle's tower outputs) ends at 0.210 of its first
    loss (1.128 -> 0.237; lr 0.01: 0.281, lr 0.2 diverges); the bound asked of the GPU loop is 0.5."""
    from sylph_amd.finetune import finetune_class_codes, prior_bias
    eng = _engine()
    recs, anns, xns, labs = [], [], [], []
    for feats, ann in FR.loop_task():
        eng.import_pyramid(feats, FR.LOOP_HW)
        eng.towers()
        xns.append(_operand(eng))
        labs.append(torch.from_numpy(FR.fcos_targets_ref(ann["boxes"].numpy(), ann["classes"].numpy(), ann["image_index"].numpy(), 2,
                                                         FR.levels(FR.LOOP_HW))))
        recs.append(eng.store_record())
        anns.append(ann)
    n = FR.LOOP_CLASSES
    start = {"cls_conv": torch.zeros(n, 256, 1, 1, device="cuda"), "cls_bias": torch.full((n,), prior_bias(0.01), device="cuda")}
    codes, losses = finetune_class_codes(eng, recs, anns, start, iters=200, lr=0.05)
    ls = losses.cpu().double()
    want = FR.loop_ref(xns, labs, n, 200, 0.05)
    print(f"loss: GPU first {float(ls[0]):.6f} last {float(ls[-1]):.6f} ratio {float(ls[-1] / ls[0]):.4f}; "
          f"float64 restatement first {want[0]:.6f} last {want[-1]:.6f} ratio {want[-1] / want[0]:.4f}")
    assert want[-1] < 0.5 * want[0]
    assert math.isfinite(float(ls[-1])) and float(ls[-1]) < 0.5 * float(ls[0])
    assert abs(float(ls[0]) - want[0]) <= ROWS * 2.0 ** -23 * want[0], "the first step's loss is the restatement's (every term is positive: A is the loss)"
    # the returned dict is what the query path takes
    assert tuple(codes["cls_conv"].shape) == (n, 256, 1, 1) and tuple(codes["cls_bias"].shape) == (n,)
    eng.load_record(recs[0])
    eng.head(codes["cls_conv"], codes["cls_bias"])
    dets = eng.decode()
    assert len(dets) == 2
    # frozen rows: bit-identical, and the others move
    w0, b0 = _codes(n, seed=103)
    mask = [True, False, True, False, True]
    part, _ = finetune_class_codes(eng, recs, anns, {"cls_conv": w0, "cls_bias": b0}, iters=3, lr=0.05, trainable=mask, records_per_step=2,
                                   lr_steps=(2,))
    m = torch.tensor(mask, device="cuda")
    assert torch.equal(part["cls_conv"][~m], w0[~m]) and torch.equal(part["cls_bias"][~m], b0[~m])
    assert not torch.equal(part["cls_conv"][m], w0[m])
    eng.close()


def test_model_and_runner_refine_codes():
    """MetaOneStageDetector.finetune_class_codes on the support images (records made and released inside), from the episode's own codes
    and from the checkpoint's cls_logits rows; the returned dict feeds model(records, class_code=...); the runner's finetune= hook"""
    from sylph_amd import synthetic as W
    from sylph_amd.data import SyntheticQueryLoader, SyntheticSupportSetLoader
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    model = r.build_model(cfg, dtype="bf16")
    model.load_state_dict(W.synthetic_state_dict(0, depth=50))
    model.eval()
    sup = SyntheticSupportSetLoader(3, 2, 128, 160, seed=5)
    qry = SyntheticQueryLoader(2, 128, 160, batch_size=2, seed=6)
    _, codes0 = r._do_test_meta_learning(cfg, model, support_loader=sup, query_loader=qry)
    _, codes1 = r._do_test_meta_learning(cfg, model, support_loader=sup, query_loader=qry, finetune=dict(iters=5, lr=0.01, batch_size=4))
    assert not model.engine._records, "the support records were not released"
    assert tuple(codes1["cls_conv"].shape) == tuple(codes0["cls_conv"].shape) == (3, 256, 1, 1)
    assert not torch.equal(codes1["cls_conv"], codes0["cls_conv"]) and bool(torch.isfinite(codes1["cls_conv"]).all())
    # the model call alone, on images with instances whose frame is twice the network's: same labels as the unscaled boxes
    from sylph_amd.structures import Boxes, Instances
    batch, big = [], []
    for item in sup:
        for rec in item[0]["support_set"]:
            inst = Instances((256, 320))
            inst.gt_boxes = Boxes(rec["instances"].gt_boxes.tensor * 2)
            inst.gt_classes = torch.full((1,), int(item[0]["support_set_target"]))
            same = Instances((128, 160))
            same.gt_boxes, same.gt_classes = Boxes(rec["instances"].gt_boxes.tensor.clone()), inst.gt_classes
            batch.append({"image": rec["image"], "instances": same})
            big.append({"image": rec["image"], "instances": inst})
    ca, la = model.finetune_class_codes(batch, codes0, iters=3, lr=0.01, batch_size=3)
    cb, lb = model.finetune_class_codes(big, codes0, iters=3, lr=0.01, batch_size=3)
    assert torch.equal(la, lb) and torch.equal(ca["cls_conv"], cb["cls_conv"])
    records = model(list(qry)[0], run_type="meta_learn_cache_query")
    out = model(records, class_code=ca, run_type="meta_learn_test_instance")
    assert len(out) == 2 and all("instances" in o for o in out)
    records[0]["record"].close()
    # a base detector's own classifier rows as the starting point (class_code None), the first 40 of 60 classes kept fixed
    pre = model._pretrained_class_codes()
    n = pre["cls_conv"].shape[0]
    cp, _ = model.finetune_class_codes(batch, None, iters=2, lr=0.01, trainable=[i >= 40 for i in range(n)])
    assert torch.equal(cp["cls_conv"][:40], pre["cls_conv"][:40]) and not torch.equal(cp["cls_conv"][40:], pre["cls_conv"][40:])
    model.engine.close()


# ------------------------------------------------------------------------------------------------ 7: refusals by name
def _towers(eng):
    eng.import_pyramid(FR.pyramid(2, HW, seed=7), HW)
    eng.towers()


@pytest.mark.parametrize("what,dtype,cfg_kw,sd_kw,match", [
    ("fp32", "f32", {}, {}, "bf16 mode only"),
    ("norm none", "bf16", {"MODEL.FCOS.NORM": "none"}, {"norm": "none"}, "NORM \"none\" is not supported"),
    ("3x3 codes", "bf16", {"MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER": ["", "", 3]}, {}, "3x3 class codes"),
])
def test_refused_contexts(what, dtype, cfg_kw, sd_kw, match):
    eng = _engine(dtype, cfg=_cfg(**cfg_kw), sd=_sd(**sd_kw), taps=False)
    _towers(eng)
    z = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match=match):
        eng.fcos_targets(torch.tensor([[10.0, 10.0, 60.0, 60.0]]), z, z)
    with pytest.raises(RuntimeError, match=match):
        eng.cls_grad(torch.full((ROWS,), -1, dtype=torch.int32, device="cuda"), torch.zeros(2, 256, device="cuda"), None)
    eng.close()


def test_refused_roi_encoder():
    from sylph_amd import synthetic as W
    sd = dict(_sd())
    sd.update(W.roi_encoder_state_dict(seed=4))
    eng = _engine("bf16", cfg=_roienc_cfg(), sd=sd, taps=False)
    _towers(eng)
    z = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROIEncoder"):
        eng.fcos_targets(torch.tensor([[10.0, 10.0, 60.0, 60.0]]), z, z)
    eng.close()


def test_refused_arguments(small):
    eng = small["eng"]
    eng.load_record(small["rec"])
    bx = torch.tensor([[10.0, 10.0, 60.0, 60.0], [20.0, 20.0, 90.0, 90.0]])
    with pytest.raises(ValueError, match="gt_image is not sorted"):
        eng.fcos_targets(bx, torch.tensor([0, 1]), torch.tensor([1, 0]))
    w, b = _codes(5, seed=104)
    lab = _labels(5)
    lab[0] = 5
    with pytest.raises(ValueError, match="a label >= N"):
        eng.cls_grad(lab.cuda(), w, b)
    with pytest.raises(ValueError, match="3x3 class codes are not supported"):
        eng.cls_grad(lab.cuda(), torch.zeros(5, 256, 3, 3), b)
