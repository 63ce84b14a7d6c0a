"""Box-branch fine-tuning on the GPU (csrc/box_finetune.hip through Engine.box_samples / box_grad / set_box_branch and
sylph_amd.finetune.finetune_box_branch), on the synthetic head over imported pyramids.

Yardsticks: tests/box_finetune_ref.py.  Samples (info, targets) and patches are compared exactly.  The gradient is checked stage by stage,
each against a bound that can be derived (box_finetune_ref's docstring):
  stage 1  z_out against float64 on the same bf16 operands: |err| <= 2304 2^-23 sum |x| |w| per element
  stage 2  g_out against the float64 formulas at the kernel's own z_out: |err| <= G_ROUNDINGS 2^-24 T
  stage 3  grad_w / grad_b / grad_scales / sums against float64 sums of the kernel's own g_out (fp32 values, no operand split: the products
           run on the VALU) with the bf16 patches: |err| <= n 2^-23 sum |g x|
Everything else is bit equality between two runs of the library."""
import os

import numpy as np
import pytest
import torch

import box_finetune_ref as BR
import finetune_ref as FR
from test_hip_parity import _cfg, _roienc_cfg

pytestmark = pytest.mark.gpu
HW = (128, 160)
SIZES = [(128, 153), (123, 160)]
CASES = ["a_on", "a_off", "b_on", "c_on", "d_on"]
SMALL_SOI = [8.0, 16.0, 32.0, 64.0]
QUALITIES = {"ctrness": ["ctrness"], "iou": ["iou"], "both": ["ctrness", "iou"]}
P = "proposal_generator.fcos_head"


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


def _operand_levels(eng):
    """the normalised last bbox tower layer of the current fresh batch as the prediction pass reads it: per level (B, 256, h, w), host"""
    from oracle import bf16 as OB16
    ys, cfs = eng.export_tower(1, 3)
    return [OB16.gn_apply(y.cpu(), cf.cpu()) for y, cf in zip(ys, cfs)]


def _codes(n, seed, scale=2.5):
    from sylph_amd import synthetic as W
    c = W.synthetic_codes(n, seed=seed, scale=scale)
    return c["cls_conv"].cuda(), c["cls_bias"].cuda()


@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(os.path.join(golden_dir, "g13_box_losses.npz"))


@pytest.fixture(scope="module")
def small():
    """one engine, the two-image ragged 128 x 160 batch (856 rows), towers run, the operand values of its bbox tower"""
    eng = _engine()
    feats = FR.pyramid(2, HW, seed=7)
    eng.import_pyramid(feats, HW, SIZES)
    eng.towers()
    yield {"eng": eng, "feats": feats, "xn": _operand_levels(eng)}
    eng.close()


@pytest.fixture(scope="module")
def big():
    """the three-image 256 x 320 batch of test_targets_random_boxes_three_images with its random boxes: the bank, its host copies"""
    hw = (256, 320)
    eng = _engine()
    eng.import_pyramid(FR.pyramid(3, hw, seed=8), hw)
    eng.towers()
    ann = FR.random_boxes(3, 40, hw, 20, seed=9, lo=4.0, hi=300.0)
    bank = eng.box_samples(ann["boxes"], ann["classes"], ann["image_index"])
    yield {"eng": eng, "hw": hw, "ann": ann, "bank": bank, "xn": _operand_levels(eng)}
    eng.close()


class _train_cfg:
    """MODEL.FCOS training settings of an engine, changed for one block"""

    def __init__(self, eng, **kw):
        self.eng, self.kw = eng, kw

    def __enter__(self):
        self.keep = dict(self.eng.fcos_train)
        self.eng.fcos_train.update(self.kw)

    def __exit__(self, *a):
        self.eng.fcos_train.clear()
        self.eng.fcos_train.update(self.keep)


# ------------------------------------------------------------------------------------------------ 1: targets and order
@pytest.mark.parametrize("soi", ["default", "small"])
@pytest.mark.parametrize("case", CASES)
def test_samples_golden_batch(small, g13, case, soi):
    eng = small["eng"]
    cs = bool(g13[f"{case}_center_sample"])
    sizes = SMALL_SOI if soi == "small" else [64.0, 128.0, 256.0, 512.0]
    bx, cl, im = g13[f"{case}_boxes"], g13[f"{case}_classes"], g13[f"{case}_image"]
    with _train_cfg(eng, center_sample=cs, sizes_of_interest=sizes):
        bank = eng.box_samples(torch.from_numpy(bx), torch.from_numpy(cl), torch.from_numpy(im))
    info, targets, _ = BR.box_samples_ref(bx, cl, im, 2, FR.levels(HW), soi=sizes, center_sample=cs)
    per_level = np.bincount(info[:, 1], minlength=5)
    print(f"{case} {soi}: {len(info)} samples, per level {per_level.tolist()}")
    assert bank.n == bank.count == len(info) and not bank.overflow
    assert len(info) > 0 or soi == "small", "every golden case has positives under the default sizes of interest"
    assert np.array_equal(bank.info.cpu().numpy(), info)
    assert np.array_equal(bank.targets.cpu().numpy(), targets)
    if soi == "default":  # the restatement is pinned to the reference on these very cases (tests/test_box_finetune_cpu.py)
        ref_labels = np.concatenate([g13[f"{case}_labels{l}"] for l in range(5)], 1)  # (2, 428): per image the tower output's row order
        assert np.array_equal(info[:, 3], ref_labels[info[:, 0] // 428, info[:, 0] % 428]), "classes differ from the reference's labels"
    if case in ("a_on", "a_off", "c_on"):
        assert not np.any(info[:, 0] >= 428), "image 1 must contribute no sample (no box / an empty sample region)"
    if soi == "small" and case == "a_off":
        assert per_level[4] > 0 and per_level[3] > 0 and per_level[2] > 0 and per_level[0] > 0, "the 1 x 2 and 2 x 3 maps must hold positives"


def test_samples_random_boxes_three_images(big):
    eng, hw, ann = big["eng"], big["hw"], big["ann"]
    levels_seen = set()
    for cs, sizes in ((True, None), (False, None), (True, SMALL_SOI)):
        kw = {"center_sample": cs}
        if sizes:
            kw["sizes_of_interest"] = sizes
        with _train_cfg(eng, **kw):
            bank = eng.box_samples(ann["boxes"], ann["classes"], ann["image_index"])
            labels, npos = eng.fcos_targets(ann["boxes"], ann["classes"], ann["image_index"])
        info, targets, _ = BR.box_samples_ref(ann["boxes"].numpy(), ann["classes"].numpy(), ann["image_index"].numpy(), 3, FR.levels(hw),
                                              center_sample=cs, **({"soi": sizes} if sizes else {}))
        assert bank.n == len(info) == int(npos) > (100 if sizes is None else 0)
        assert np.array_equal(bank.info.cpu().numpy(), info) and np.array_equal(bank.targets.cpu().numpy(), targets)
        lab = labels.cpu().numpy()
        assert np.array_equal(np.nonzero(lab >= 0)[0], info[:, 0]) and np.array_equal(lab[info[:, 0]], info[:, 3]), "the samples are fcos_targets' positives"
        levels_seen |= set(info[:, 1].tolist())
    assert levels_seen == {0, 1, 2, 3, 4}


# ------------------------------------------------------------------------------------------------ 2: patches
def test_patches_are_the_operand_values(small, big, g13):
    eng = small["eng"]
    bx, cl, im = g13["a_off_boxes"], g13["a_off_classes"], g13["a_off_image"]
    with _train_cfg(eng, center_sample=False, sizes_of_interest=SMALL_SOI):
        bank = eng.box_samples(torch.from_numpy(bx), torch.from_numpy(cl), torch.from_numpy(im))
    info = bank.info.cpu().numpy()
    shapes = FR.levels(HW)
    want = BR.patches_ref(small["xn"], info, shapes)
    got = bank.patches.float().cpu()
    assert got.shape == want.shape and torch.equal(got, want), f"{int((got != want).sum())} patch values differ"
    # where the samples sit: corners, edges, the 1 x 2 and the 2 x 3 map
    off = np.cumsum([0] + [h * w for h, w in shapes])
    kinds = set()
    for p, (row, l, _, _) in enumerate(info):
        h, w = shapes[l]
        y, x = divmod(int(row) % 428 - off[l], w)
        ey, ex = y in (0, h - 1), x in (0, w - 1)
        kinds.add("corner" if ey and ex else ("edge" if ey or ex else "inner"))
        outside = [(ky, kx) for ky in range(3) for kx in range(3) if not (0 <= y + ky - 1 < h and 0 <= x + kx - 1 < w)]
        for ky, kx in outside:
            assert float(got[p, ky, kx].abs().max()) == 0.0
        if (h, w) == (1, 2):
            assert len(outside) == 7
            kinds.add("1x2")
        if (h, w) == (2, 3):
            kinds.add("2x3")
    assert kinds == {"corner", "edge", "inner", "1x2", "2x3"}, kinds
    assert float(want.abs().max()) > 0
    # the larger batch, every level
    b3 = big["bank"]
    assert torch.equal(b3.patches.float().cpu(), BR.patches_ref(big["xn"], b3.info.cpu().numpy(), FR.levels(big["hw"])))


# ------------------------------------------------------------------------------------------------ 3: capacity
def test_capacity_and_empty_inputs(small, g13):
    eng = small["eng"]
    bx, cl, im = (torch.from_numpy(g13[f"a_off_{k}"]) for k in ("boxes", "classes", "image"))
    with _train_cfg(eng, center_sample=False):
        full = eng.box_samples(bx, cl, im)
        n = full.n
        assert n > 2
        out = (torch.full((n + 1, 3, 3, 256), 7.0, device="cuda", dtype=torch.bfloat16), torch.full((n + 1, 4), 7.0, device="cuda"),
               torch.full((n + 1, 4), 7, device="cuda", dtype=torch.int32))
        cut = eng.box_samples(bx, cl, im, max_samples=n - 1, out=out, allow_overflow=True)
        assert cut.overflow and cut.count == n and cut.n == n - 1
        assert torch.equal(cut.info, full.info[:n - 1]) and torch.equal(cut.targets, full.targets[:n - 1]) and torch.equal(cut.patches, full.patches[:n - 1])
        for t in out:  # the canary behind the capacity: rows n - 1 and n
            assert bool((t[n - 1:].float() == 7.0).all()), "a row past max_samples was written"
        with pytest.raises(RuntimeError, match="exceed max_samples"):
            eng.box_samples(bx, cl, im, max_samples=n - 1)
    none = eng.box_samples(torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    assert none.n == none.count == 0 and not none.overflow
    w, b, s = _stack(eng.box_branch())
    zero = eng.box_grad(none, w, b, s)
    assert all(float(zero[k].abs().max()) == 0.0 for k in ("sums", "grad_w", "grad_b", "grad_scales"))


def _stack(branch):
    from sylph_amd.finetune import stack_box_branch
    return stack_box_branch(branch)


# ------------------------------------------------------------------------------------------------ 4: served values
def test_z_out_reproduces_the_served_predictions(big):
    eng, bank = big["eng"], big["bank"]
    eng.head(*_codes(5, seed=21))
    _, reg, ctr, iou = eng.export_head()
    rows = bank.info[:, 0].long().cpu()
    served = torch.cat([FR.rows_of([t.cpu() for t in ts])[rows] for ts in (reg, ctr, iou)], 1).double()
    w, b, s = _stack(eng.box_branch())
    z = eng.box_grad(bank, w, b, s, debug=True)["z"].cpu().double()
    sl = s.double()[bank.info[:, 1].long().cpu()]
    mine = torch.cat([torch.relu(sl[:, None] * z[:, :4]), z[:, 4:]], 1)
    x = bank.patches.float().cpu().reshape(bank.n, -1).double()
    A = x.abs() @ BR.pack_w(w).double().abs().t()
    bound = 2304 * 2.0 ** -23 * A * torch.cat([sl[:, None].expand(-1, 4), torch.ones(bank.n, 2, dtype=torch.float64)], 1)
    ratio = float(((mine - served).abs() / bound).max())
    print(f"served values at {bank.n} positives: worst |err| / (2304 2^-23 sum |x||w|) = {ratio:.4g}")
    assert float(served[:, :4].max()) > 0 and ratio <= 1.0


# ------------------------------------------------------------------------------------------------ 5: the gradient, stage by stage
def _test_branch(bank_x, info, tau, quality, mask):
    """Branch weights under which no sample sits within the stage-1 bound of a kink, so that the float64 restatement and the kernel stay
    on one branch of relu / min / max (and of the 0.3 IoU mask): small regression weights around per-side biases, and a NEGATIVE scale on
    level 1 so that its samples sit behind the ReLU.  The first of 20 seeded candidates whose margin holds; the caller asserts it."""
    lv = info[:, 1].long()
    for seed in range(20):
        g = torch.Generator().manual_seed(900 + seed)
        w = torch.cat([torch.randn(4, 256, 3, 3, generator=g) * 2e-4, torch.randn(2, 256, 3, 3, generator=g) * 0.02])
        b = torch.cat([0.4 + torch.rand(4, generator=g) * 3.0, torch.randn(2, generator=g) * 0.5])
        s = torch.tensor([1.0, -0.9, 1.1, 1.3, 0.8]) + torch.rand(5, generator=g) * 0.05
        z = bank_x @ BR.pack_w(w).double().t() + b.double()[None]
        t = BR.box_grad_terms(z, tau, s.double()[lv], quality, mask)
        bound = 2304 * 2.0 ** -23 * (bank_x.abs() @ BR.pack_w(w).double().abs().t())
        side = (s.double()[lv].abs()[:, None] * bound[:, :4]).max(1)[0]
        ok = bool((t["margin"] > 2 * side).all())
        if mask:
            ok = ok and bool(((t["iou_value"] - 0.3).abs() > 1e-3).all())
        if ok:
            return w, b, s, side
    raise AssertionError("no candidate branch keeps every sample away from the kinks")


def _bank_slices(big):
    from sylph_amd.engine import BoxSamples
    bank = big["bank"]
    reps = (5000 + bank.n - 1) // bank.n
    return {"1": bank.select(torch.arange(1, device="cuda")), "33": bank.select(torch.arange(33, device="cuda") + 7),
            "65": bank.select(torch.arange(65, device="cuda") + 100), "bank": bank, "tiled": BoxSamples.cat([bank] * reps)}


@pytest.mark.parametrize("which", ["1", "33", "65", "bank", "tiled"])
@pytest.mark.parametrize("qn, mask", [("ctrness", False), ("iou", False), ("both", False), ("both", True), ("iou", True), ("ctrness", True)])
def test_gradient_stage_by_stage(big, which, qn, mask):
    eng, q = big["eng"], QUALITIES[qn]
    bank = _bank_slices(big)[which]
    n = bank.n
    if which == "tiled":
        assert n >= 5000 and (n + 31) // 32 > 64, "several units, more than one reduce pass sums"
    x = bank.patches.float().cpu().reshape(n, -1).double()
    info, tau = bank.info.cpu(), bank.targets.cpu().double()
    lv = info[:, 1].long()
    w, b, s, side = _test_branch(x, info, tau, q, mask)
    out = eng.box_grad(bank, w, b, s, debug=True, quality=q, iou_mask=mask)
    z, g = out["z"].cpu().double(), out["g"].cpu().double()
    wq, sl = BR.pack_w(w).double(), s.double()[lv]
    # stage 1
    z64 = x @ wq.t() + b.double()[None]
    b1 = 2304 * 2.0 ** -23 * (x.abs() @ wq.abs().t())
    r1 = float(((z - z64).abs() / b1).max())
    # the margin: at the float64 z and at the kernel's z alike, every side is further from a kink than the stage-1 bound
    t64 = BR.box_grad_terms(z64, tau, sl, q, mask)
    t = BR.box_grad_terms(z, tau, sl, q, mask)
    assert bool((t64["margin"] > 2 * side).all()) and bool((t["margin"] > side).all()), "a sample sits within the stage-1 bound of a kink"
    if which in ("bank", "tiled"):
        assert bool((sl[:, None] * z[:, :4] < 0).any()) and bool((sl[:, None] * z[:, :4] > 0).any()), "some samples must sit behind the ReLU"
    # stage 2
    b2 = BR.G_ROUNDINGS * 2.0 ** -24 * t["T"]
    live = t["T"] > 0
    assert bool((g[~live] == 0).all()), "a channel that receives no gradient must hold exact zeros"
    r2 = float(((g - t["g"]).abs()[live] / b2[live]).max())
    # stage 3: sums of the kernel's own g (and of the restatement's per-sample losses) in float64
    gw64 = (g.t() @ x).reshape(6, 3, 3, 256).permute(0, 3, 1, 2)
    A_w = (g.abs().t() @ x.abs()).reshape(6, 3, 3, 256).permute(0, 3, 1, 2)
    gscale_k = (g[:, :4] * z[:, :4] / sl[:, None]).sum(1)  # d loss / d scale from the kernel's own g and z
    onehot = torch.nn.functional.one_hot(lv, 5).double()
    bn = n * 2.0 ** -23
    r3 = {"grad_w": float(((out["grad_w"].cpu().double() - gw64).abs() / (bn * A_w).clamp(min=1e-300)).max()),
          "grad_b": float(((out["grad_b"].cpu().double() - g.sum(0)).abs() / (bn * g.abs().sum(0)).clamp(min=1e-300)).max()),
          # per term one more rounding than the sum's own (g z / s is formed in fp32 before it is added): 4 sides x 3 roundings
          "grad_scales": float(((out["grad_scales"].cpu().double() - onehot.t() @ gscale_k).abs() /
                                ((bn + 12 * 2.0 ** -24) * (onehot.t() @ (g[:, :4] * z[:, :4] / sl[:, None]).abs().sum(1))).clamp(min=1e-300)).max())}
    sums64 = torch.stack([t["loc"].sum(), t["ctr"].sum(), t["iou"].sum(), t["ctr_t"].sum()])
    # a sum of n terms, each the end of a chain of at most G_ROUNDINGS fp32 roundings (exp / log1p within 2 ulp); the sums of absolute
    # terms: wgt (1 + iou + |ac - au| / ac) <= 3 wgt; max(z, 0) + |z| t + log1p(e) <= 2 |z| + 1; the centerness targets themselves
    wgt = t["ctr_t"] if "ctrness" in q else torch.ones_like(t["ctr_t"])
    A_s = torch.stack([3 * wgt.sum(), (2 * z[:, 4].abs() + 1).sum(), (2 * z[:, 5].abs() + 1).sum(), t["ctr_t"].sum()])
    r3["sums"] = float(((out["sums"].cpu().double() - sums64).abs() / ((bn + BR.G_ROUNDINGS * 2.0 ** -24) * A_s)).max())
    print(f"n = {n} {qn} mask {mask}: worst ratio to the bound: stage 1 {r1:.4g}, stage 2 {r2:.4g}, stage 3 {r3}")
    assert float(A_w.min()) >= 0 and float(gw64.abs().max()) > 1e-4, "the comparison proves nothing"
    assert r1 <= 1.0, f"z_out misses its bound by a factor {r1:.3g}"
    assert r2 <= 1.0, f"g_out misses its bound by a factor {r2:.3g}"
    for k, r in r3.items():
        assert r <= 1.0, f"{k} misses its bound by a factor {r:.3g}"


# ------------------------------------------------------------------------------------------------ 6: same bits
def test_same_bits_twice_and_on_any_grid(big, monkeypatch):
    eng = big["eng"]
    bank = _bank_slices(big)["tiled"]
    w, b, s = _stack(eng.box_branch())
    first = eng.box_grad(bank, w, b, s, debug=True)
    runs = [eng.box_grad(bank, w, b, s, debug=True)]
    for cap in ("1", "3"):
        monkeypatch.setenv("SYLPH_BOX_GRAD_BLOCKS", cap)
        runs.append(eng.box_grad(bank, w, b, s, debug=True))
    monkeypatch.delenv("SYLPH_BOX_GRAD_BLOCKS")
    for other in runs:
        for k in first:
            assert torch.equal(first[k], other[k]), f"{k}: other bits"
    assert float(first["grad_w"].abs().max()) > 0
    again = eng.box_samples(big["ann"]["boxes"], big["ann"]["classes"], big["ann"]["image_index"])
    for k in ("patches", "targets", "info"):
        assert torch.equal(getattr(again, k), getattr(big["bank"], k))


# ------------------------------------------------------------------------------------------------ 7: install
def _other_branch(eng, seed=77):
    from sylph_amd.finetune import split_box_branch
    w, b, s = _stack(eng.box_branch())
    g = torch.Generator().manual_seed(seed)
    return split_box_branch(w + torch.randn(w.shape, generator=g) * 0.01, b + torch.randn(b.shape, generator=g) * 0.2,
                            s * (1 + torch.rand(s.shape, generator=g) * 0.2))


def _step(eng, feats, codes):
    eng.import_pyramid(feats, HW, SIZES)
    eng.towers()
    eng.head(*codes)
    return eng.export_head(), eng.decode()


def _same(a, b):
    (ha, da), (hb, db) = a, b
    heads = all(torch.equal(x, y) for xs, ys in zip(ha, hb) for x, y in zip(xs, ys))
    dets = all(torch.equal(x[k], y[k]) for x, y in zip(da, db) for k in ("pred_boxes", "scores", "pred_classes", "fpn_levels", "locations", "cand_index"))
    return heads and dets


def test_install_is_a_context_finalized_with_the_branch():
    feats, codes = FR.pyramid(2, HW, seed=7), _codes(5, seed=22, scale=3.0)
    eng = _engine(taps=False)
    base = _step(eng, feats, codes)
    rec = eng.store_record()
    assert all(d["scores"].numel() > 0 for d in base[1]), "no detection: the comparison proves nothing"
    branch = _other_branch(eng)
    sd = dict(_sd())
    for k, v in branch.items():
        assert f"{P}.{k}" in sd and sd[f"{P}.{k}"].shape == v.shape
        sd[f"{P}.{k}"] = v
    other = _engine(sd=sd, taps=False)
    want = _step(other, feats, codes)
    assert eng.box_branch_shape()[2] == 0
    eng.set_box_branch(branch)
    assert eng.box_branch_shape()[2] != 0
    assert all(torch.equal(v, eng.box_branch()[k]) for k, v in branch.items())
    with pytest.raises(RuntimeError, match="no current batch"):
        eng.towers()
    got = _step(eng, feats, codes)
    assert _same(got, want), "the installed branch does not give the bits of an engine loaded with it"
    assert not _same(got, base)
    assert all(torch.equal(x, y) for x, y in zip(got[0][0], base[0][0])), "the logits must not change"
    with pytest.raises(RuntimeError, match="another box branch"):
        eng.load_record(rec)
    eng.reset_box_branch()
    assert eng.box_branch_shape()[2] == 0
    assert _same(_step(eng, feats, codes), base), "reset does not return the baseline's bits"
    eng.load_record(rec)
    eng.head(*codes)
    assert _same((eng.export_head(), eng.decode()), base)
    eng.close()
    other.close()


# ------------------------------------------------------------------------------------------------ 8: loop, model, runner
def test_loop_lowers_the_three_losses_and_keeps_frozen_parts(big):
    """100 steps on the 256 x 320 bank, lr 5e-4 with momentum 0.9.  The Hessian of a linear layer on patches of 2304 values of mean
    square ~0.3 has eigenvalues up to ~700 x the loss curvature (<= 1), and SGD with momentum m is stable below 2 (1 + m) / lambda ~ 5e-3:
    a tenth of that.
    The start is the engine's own box regression with the two quality heads as a new head starts (zero weights, the prior bias
    -log(99), fcos.py:432-433).  From the synthetic checkpoint's own quality heads the IoU-quality loss does NOT end below its first
    value (measured: loc 0.908 -> 0.616, ctr 0.713 -> 0.676, iou 0.6535 -> 0.6205 after three steps -> 0.6610 after 100): a BCE against
    soft targets is bounded below by the targets' entropy, and as the boxes improve the IoU targets rise from ~0.25 towards 0.5, where
    that floor peaks at log 2 = 0.693.  That is the loss's, not the kernel's; the stage tests above pin the gradient."""
    import math
    from sylph_amd.finetune import finetune_box_branch
    eng, bank = big["eng"], big["bank"]
    start = eng.box_branch()
    for head in ("ctrness", "iou_overlap"):
        start[f"{head}.weight"] = torch.zeros_like(start[f"{head}.weight"])
        start[f"{head}.bias"] = torch.full_like(start[f"{head}.bias"], -math.log(99.0))
    with _train_cfg(eng, box_quality=["ctrness", "iou"]):
        branch, losses = finetune_box_branch(eng, bank, start, iters=100, lr=5e-4)
    ls = losses.cpu()
    print(f"(loc, ctr, iou): first {ls[0].tolist()} last {ls[-1].tolist()}")
    assert bool(torch.isfinite(ls).all()) and bool((ls[-1] < ls[0]).all()), "each of the three losses must end below its first value"
    assert sorted(branch) == sorted(start) and not torch.equal(branch["bbox_pred.weight"], start["bbox_pred.weight"])
    with _train_cfg(eng, box_quality=["ctrness"]):
        part, _ = finetune_box_branch(eng, bank, start, iters=3, lr=5e-4, samples_per_step=64, lr_steps=(2,))
    assert torch.equal(part["iou_overlap.weight"], start["iou_overlap.weight"]) and torch.equal(part["iou_overlap.bias"], start["iou_overlap.bias"])
    assert not torch.equal(part["ctrness.weight"], start["ctrness.weight"]) and not torch.equal(part["scales.0.scale"], start["scales.0.scale"])
    with _train_cfg(eng, box_quality=["iou"]):
        part, _ = finetune_box_branch(eng, bank, start, iters=2, lr=5e-4)
    assert torch.equal(part["ctrness.weight"], start["ctrness.weight"]) and not torch.equal(part["iou_overlap.weight"], start["iou_overlap.weight"])


def _mean_giou(eng, bank):
    """mean GIoU between the served regression at the bank's positives and their targets, on the current batch after a head call"""
    _, reg, _, _ = eng.export_head()
    served = FR.rows_of([t.cpu() for t in reg])[bank.info[:, 0].long().cpu()].double()
    return float(BR.compute_ious(served, bank.targets.cpu().double())[1].mean())


def test_model_and_runner_train_and_install_the_branch():
    from sylph_amd import synthetic as W
    from sylph_amd.data import SyntheticQueryLoader, SyntheticSupportSetLoader
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    model = r.build_model(cfg, dtype="bf16")
    model.load_state_dict(W.synthetic_state_dict(0, depth=50))
    model.eval()
    eng = model.engine
    sup = SyntheticSupportSetLoader(3, 2, 128, 160, seed=5)
    qry = SyntheticQueryLoader(2, 128, 160, batch_size=2, seed=6)
    batch = r._support_batch(sup)
    assert len(batch) == 6
    codes = _codes(3, seed=23)

    def giou_now():
        model._run_backbone(batch)
        eng.head(*codes)
        ann = model._record_annotations({"inputs": [dict(instances=x["instances"]) for x in batch]})
        return _mean_giou(eng, eng.box_samples(ann["boxes"], ann["classes"], ann["image_index"]))
    before = giou_now()
    start = eng.box_branch()
    branch, losses = model.finetune_box_branch(batch, iters=60, lr=5e-4, batch_size=4)
    assert all(torch.equal(v, eng.box_branch()[k]) for k, v in start.items()), "finetune_box_branch must not install the branch"
    model.set_box_branch(branch)
    after = giou_now()
    ls = losses.cpu()
    print(f"mean GIoU at the positives: {before:.4f} -> {after:.4f}; loc loss {float(ls[0, 0]):.4f} -> {float(ls[-1, 0]):.4f}")
    assert after > before
    model.set_box_branch(None)
    # the runner's hook: trains, installs for the query loop, restores
    res, _ = r._do_test_meta_learning(cfg, model, support_loader=sup, query_loader=qry,
                                      finetune=dict(iters=2, lr=0.01, batch_size=4, box_branch=dict(iters=3, lr=5e-4, batch_size=4)))
    assert eng.box_branch_shape()[2] == 0
    assert all(torch.equal(v, eng.box_branch()[k]) for k, v in start.items()), "the branch after the run is the checkpoint's, bit for bit"
    eng.close()


# ------------------------------------------------------------------------------------------------ 9: refusals by name
def _towers(eng):
    eng.import_pyramid(FR.pyramid(2, HW, seed=7), HW)
    eng.towers()


_BOX = (torch.tensor([[10.0, 10.0, 60.0, 60.0]]), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))


@pytest.mark.parametrize("what,dtype,cfg_kw,sd_kw,match", [
    ("fp32", "f32", {}, {}, "bf16 mode only"),
    ("f32s", "f32s", {}, {}, "bf16 mode only"),
    ("norm none", "bf16", {"MODEL.FCOS.NORM": "none"}, {"norm": "none"}, "NORM \"none\" is not supported"),
])
def test_refused_contexts(what, dtype, cfg_kw, sd_kw, match):
    from sylph_amd.engine import BoxSamples
    eng = _engine(dtype, cfg=_cfg(**cfg_kw), sd=_sd(**sd_kw), taps=False)
    _towers(eng)
    with pytest.raises(RuntimeError, match=match):
        eng.box_samples(*_BOX)
    empty = BoxSamples(torch.zeros(0, 3, 3, 256, device="cuda", dtype=torch.bfloat16), torch.zeros(0, 4, device="cuda"),
                       torch.zeros(0, 4, device="cuda", dtype=torch.int32))
    with pytest.raises(RuntimeError, match=match):
        eng.box_grad(empty, torch.zeros(6, 256, 3, 3), torch.zeros(6), torch.ones(5))
    with pytest.raises(RuntimeError, match=match):
        eng.set_box_branch(eng.box_branch())
    eng.close()


def test_refused_roi_encoder_and_loss_type():
    from sylph_amd import synthetic as W
    sd = dict(_sd())
    sd.update(W.roi_encoder_state_dict(seed=4))
    eng = _engine("bf16", cfg=_roienc_cfg(), sd=sd, taps=False)
    _towers(eng)
    with pytest.raises(RuntimeError, match="ROIEncoder"):
        eng.box_samples(*_BOX)
    eng.close()
    eng = _engine(taps=False)
    _towers(eng)
    with _train_cfg(eng, loc_loss_type="iou"):
        with pytest.raises(NotImplementedError, match="LOC_LOSS_TYPE"):
            eng.box_samples(*_BOX)
    eng.close()


def test_refused_record_and_shapes(small):
    eng = small["eng"]
    rec = eng.store_record()
    eng.load_record(rec)
    with pytest.raises(RuntimeError, match="query record"):
        eng.box_samples(*_BOX)
    eng.import_pyramid(small["feats"], HW, SIZES)
    with pytest.raises(RuntimeError, match="towers have not run"):
        eng.box_samples(*_BOX)
    eng.towers()
    bank = eng.box_samples(*_BOX)
    with pytest.raises(ValueError, match="the box branch is w"):
        eng.box_grad(bank, torch.zeros(5, 256, 3, 3), torch.zeros(5), torch.ones(5))
    with pytest.raises(ValueError, match="gt_image is not sorted"):
        eng.box_samples(torch.tensor([[10.0, 10.0, 60.0, 60.0]] * 2), torch.tensor([0, 1]), torch.tensor([1, 0]))
    br = eng.box_branch()
    br["bbox_pred.weight"] = br["bbox_pred.weight"][:3]
    with pytest.raises(ValueError, match="the box branch is w"):
        eng.set_box_branch(br)
    rec.close()
