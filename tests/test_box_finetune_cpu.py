"""Box-branch fine-tuning without a GPU: the float64 restatement of tests/box_finetune_ref.py against the reference's own numbers
(tests/golden/g13_box_losses.npz, written by tests/golden/gen_box_finetune_golden.py from FCOSOutputs._get_ground_truth and
FCOSOutputs.fcos_losses), its hand-written derivative against torch autograd, the optimiser, and the runner's refusals."""
import os

import numpy as np
import pytest
import torch

import box_finetune_ref as BR
import finetune_ref as FR

HW = (128, 160)
CASES = ["a_on", "a_off", "b_on", "c_on", "d_on"]
QUALITIES = {"ctrness": ["ctrness"], "iou": ["iou"], "both": ["ctrness", "iou"]}


@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(os.path.join(golden_dir, "g13_box_losses.npz"))


@pytest.mark.parametrize("case", CASES)
def test_targets_reproduce_the_reference(g13, case):
    """labels and regression targets of every location, per image and level: exact"""
    cs = bool(g13[f"{case}_center_sample"])
    info, targets, tables = BR.box_samples_ref(g13[f"{case}_boxes"], g13[f"{case}_classes"], g13[f"{case}_image"], 2, FR.levels(HW), center_sample=cs)
    bg = int(g13["back_ground_id"])
    n_pos = 0
    for l in range(5):
        lab, reg = g13[f"{case}_labels{l}"], g13[f"{case}_reg_targets{l}"]
        for b in range(2):
            k, r = tables[(b, l)]
            want_pos = lab[b] != bg
            assert np.array_equal(k >= 0, want_pos), f"{case}: positives of image {b} level {l}"
            assert np.array_equal(g13[f"{case}_classes"][k[want_pos]], lab[b][want_pos])
            assert np.array_equal(r, reg[b]), f"{case}: regression targets of image {b} level {l}"
            n_pos += int(want_pos.sum())
    assert len(info) == n_pos > 0 and np.all(np.diff(info[:, 0]) > 0)
    # the sample list is those positives in row order, with the same targets
    rows = FR.levels(HW)
    off = np.cumsum([0] + [h * w for h, w in rows])
    for (row, l, k, c), t in zip(info, targets):
        b, i = divmod(int(row), int(off[-1]))
        assert off[l] <= i < off[l + 1]
        assert np.array_equal(t, g13[f"{case}_reg_targets{l}"][b][i - off[l]]) and c == g13[f"{case}_classes"][k]
    if case == "c_on":
        assert not np.any(info[:, 0] >= off[-1]), "image 1 of case c has an empty sample region"
    if case.startswith("a_"):
        assert not np.any(info[:, 0] >= off[-1]), "image 1 of case a has no box"


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("qn", list(QUALITIES))
@pytest.mark.parametrize("mask", [0, 1])
def test_losses_reproduce_the_reference(g13, case, qn, mask):
    """float64 restatement against the reference's float32 evaluation: each loss is a sum of n terms divided by a sum of at most n terms,
    every term a chain of about 16 fp32 operations -> |err| <= (2 n + 32) 2^-24 of the normalised sum of absolute terms"""
    q = QUALITIES[qn]
    f = lambda k: torch.from_numpy(g13[f"{case}_{k}"]).double()
    reg, ctr, iou, tau = f("pos_reg_pred"), f("pos_ctr_pred"), f("pos_iou_pred"), f("pos_reg_targets")
    n = reg.shape[0]
    sums = BR.box_losses(reg, ctr, iou, tau, q, bool(mask))
    got = dict(zip(("loc", "ctr", "iou"), BR.normalised(sums, n, q)))
    returned = {"loc": True, "ctr": "ctrness" in q, "iou": "iou" in q}
    tol = (2 * n + 32) * 2.0 ** -24
    for k in ("loc", "ctr", "iou"):
        want = float(g13[f"{case}_{qn}_{mask}_{k}"])
        if not returned[k]:
            assert np.isnan(want), f"fcos_losses returned loss_fcos_{k} under BOX_QUALITY {q}"
            continue
        print(f"{case} {qn} mask {mask} {k}: {got[k]:.9g} reference {want:.9g}")
        assert abs(got[k] - want) <= tol * max(abs(want), 1.0), (k, got[k], want)
    # the golden's own positives are fcos_losses' (level-major): the per-sample restatement gives the same sums
    scale = torch.ones(n, dtype=torch.float64)
    z = torch.cat([reg, ctr[:, None], iou[:, None]], 1)  # reg > 0: relu(1 * z) is the prediction itself
    t = BR.box_grad_terms(z, tau, scale, q, bool(mask))
    for k in ("loc", "ctr", "iou"):
        assert abs(float(t[k].sum()) - float(sums[k])) <= 1e-12 * max(1.0, abs(float(sums[k])))
    if mask:
        assert bool((t["iou_value"] < 0.3).any()) and bool((t["iou_value"] >= 0.3).any()), "the mask case must mask some and keep some"


def _random_task(n, cout, seed):
    g = torch.Generator().manual_seed(seed)
    tau = torch.rand(n, 4, generator=g, dtype=torch.float64) * 5 + 0.2
    z = torch.randn(n, cout, generator=g, dtype=torch.float64) * 3
    scale = 0.6 + torch.rand(n, generator=g, dtype=torch.float64)
    return z, tau, scale


@pytest.mark.parametrize("qn, cout", [("ctrness", 5), ("ctrness", 6), ("iou", 6), ("both", 6)])  # a five-channel branch has no iou_overlap
@pytest.mark.parametrize("mask", [False, True])
def test_derivative_against_autograd(qn, mask, cout):
    q = QUALITIES[qn]
    z, tau, scale = _random_task(400, cout, 7 + cout)
    t = BR.box_grad_terms(z, tau, scale, q, mask)
    keep = t["margin"] > 1e-6  # (autograd splits the derivative at a tie of min / max; no sample is that close)
    assert bool(keep.all())
    assert bool((scale[:, None] * z[:, :4] <= 0).any()), "some sides must sit behind the ReLU"
    zz, ss = z.clone().requires_grad_(True), scale.clone().requires_grad_(True)
    reg, ctr, iou = BR.branch_forward(zz, ss)
    total = BR.box_losses(reg, ctr, iou, tau, q, mask)["total"]
    gz, gs = torch.autograd.grad(total, [zz, ss])
    for name, got, want in (("g", t["g"], gz), ("gscale", t["gscale"], gs)):
        err = (got - want).abs().max() / want.abs().max()
        assert float(err) <= 1e-12, f"{name}: {float(err):.3g}"
    assert bool((t["T"] >= t["g"].abs() * (1 - 1e-12)).all()), "T bounds |g| term by term"
    if "ctrness" not in q:
        assert float(t["g"][:, 4].abs().max()) == 0.0
    if cout == 6 and "iou" not in q:
        assert float(t["g"][:, 5].abs().max()) == 0.0


def test_optimiser_keeps_frozen_parts_and_follows_the_lr_steps():
    from sylph_amd.finetune import BranchOptimizer, box_loss_norms, split_box_branch, stack_box_branch
    g = torch.Generator().manual_seed(3)
    w, b, s = torch.randn(6, 256, 3, 3, generator=g), torch.randn(6, generator=g), torch.ones(5)
    br = split_box_branch(w, b, s)
    assert sorted(br) == sorted(["bbox_pred.weight", "bbox_pred.bias", "ctrness.weight", "ctrness.bias", "iou_overlap.weight", "iou_overlap.bias"] +
                                [f"scales.{l}.scale" for l in range(5)])
    assert all(torch.equal(a, c) for a, c in zip(stack_box_branch(br), (w, b, s)))
    opt = BranchOptimizer(w, b, s, ["ctrness"], lr=0.1, momentum=0.9, weight_decay=1e-2, lr_steps=(2, 4), lr_gamma=0.5)
    sums = torch.tensor([3.0, 1.0, 1.0, 2.5])
    loc_norm, npos = box_loss_norms(sums, 7, ["ctrness"])
    assert float(loc_norm) == 2.5 and float(npos) == 7.0
    assert float(box_loss_norms(sums, 7, ["iou"])[0]) == 7.0 and float(box_loss_norms(sums * 0, 0, ["ctrness"])[0]) == pytest.approx(1e-6)
    lrs = []
    wr, buf = w.double().clone(), None
    for it in range(6):
        gw, gb, gs = torch.randn(6, 256, 3, 3, generator=g), torch.randn(6, generator=g), torch.randn(5, generator=g)
        lrs.append(opt.lr)
        opt.step(gw, gb, gs, loc_norm, npos)
        div = torch.tensor([2.5] * 4 + [7.0] * 2, dtype=torch.float64).reshape(6, 1, 1, 1)
        wr, buf = FR.sgd_ref(wr, gw.double() / div, buf, lrs[-1], 0.9, 1e-2)
    assert lrs == pytest.approx([0.1, 0.1, 0.05, 0.05, 0.025, 0.025])
    assert torch.equal(opt.w[5], w[5]) and torch.equal(opt.b[5], b[5]), "iou_overlap is not trained under BOX_QUALITY ['ctrness']: same bits"
    assert torch.allclose(opt.w[:5].double(), wr[:5], rtol=1e-5, atol=1e-6)
    assert not torch.equal(opt.s, s)
    frozen = BranchOptimizer(w, b, s, ["iou"], lr=0.1, train_scales=False)
    frozen.step(torch.ones_like(w), torch.ones_like(b), torch.ones_like(s), loc_norm, npos)
    assert torch.equal(frozen.s, s) and torch.equal(frozen.w[4], w[4]) and not torch.equal(frozen.w[5], w[5])


@pytest.mark.parametrize("kw, what", [(dict(cache_queries=True), "cache_queries"), (dict(fuse_repeats=True), "fuse_repeats"),
                                      (dict(shot_bank=object(), bank_draws=[(1, 0)]), "shot bank")])
def test_runner_refuses_by_name(kw, what):
    from sylph_amd.runner import MetaFCOSRunner
    ft = dict(iters=1, lr=0.01, box_branch=dict(iters=1, lr=0.01))
    with pytest.raises(NotImplementedError, match=what):
        MetaFCOSRunner()._do_test_meta_learning(None, None, finetune=ft, **kw)
