"""The bf16 PRODUCTION kernels pinned to bf16 ulps at production shapes.

The fp32-mode tests prove the layer graph (<= 1e-3 against the reference goldens / the fp32 oracle) on the exact-fp32 MFMA.
The kernels that are timed -- conv_hpipe (plain + GroupNorm-in), conv_pw / conv_igemm bf16, bottleneck64[p], stem_pool,
gn_logits, gn_taps + tap_gather -- are bf16-only.  Here each of them runs through the C ABI on the SAME operands as
oracle/bf16.py (the oracle restated with a bf16 rounding at every point where the HIP graph stores bf16): both sides
then round the same fp32 value up to summation order, so outputs must agree BIT FOR BIT except for isolated 1-ulp flips
of values sitting on a rounding boundary.  A dropped tap on a patch edge, a wrong GroupNorm coefficient on one
(image, group), a mis-addressed halo row: each is a many-ulp error on some element and fails these bounds.

Tolerances (stated, not tuned to pass):
  * a kernel with no bf16 intermediate inside (tower conv, stem): worst element <= 1 bf16 ulp OF THAT ELEMENT (floor: 1e-3 of
    the tensor's maximum, below which fp32 summation noise is no longer small against the element's own spacing) and <= 1 % of
    elements not identical;
  * several convs with bf16 intermediates in between (a bottleneck block, a ResNet stage): a flipped t1 / t2 element moves
    the next conv's fp32 sum by |w| * 2^-8 |t|, i.e. by a fraction of one bf16 ulp AT THE OUTPUT'S SCALE, whatever the
    magnitude of the output element itself (residual sums cancel): the ulp is taken at max(|element|, rms of the tensor);
    <= 2 such ulps and <= 3 % of elements not identical for ONE block (measured: 1.5-2 ulps, 0.01-0.8 %).  Through a chain
    of blocks the flips spread -- every flipped input nudges all the sums it feeds, each nudge flips the next rounding with
    probability ~ nudge / ulp -- until a large share of the elements differs by an ulp or two (measured: res3, four blocks,
    12 %, 5 ulps; res4, six blocks, 42 %, 8 ulps).  For a whole stage / the pyramid the statement is therefore about the error
    ENERGY: relative L2 error <= 2^-8 (one bf16 ulp, relative) and no element off by more than 16 ulps.  These chain tests
    check the wiring (buffers, strides, stage hand-offs); the per-block tests above them are the tight ones.  A structural
    error (dropped tap, wrong row, wrong coefficient) is O(rms): relative L2 ~ 0.1-1, > 100 ulps;
  * fp32 outputs (logits, box / ctrness / iou predictions, GroupNorm coefficients): 1e-4 of the output scale (summation order).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from bf16_ulps import assert_chain as _assert_chain, assert_ulps as _assert_ulps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W = 800, 1344
LEVELS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]


def _engine(dtype="bf16", cfg=None):
    from sylph_amd.engine import Engine
    return Engine(cfg, dtype=dtype)


def _cfg():
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    return cfg


def _routing_overrides():
    return sorted(k for k in os.environ if k.startswith(("SYLPH_CONV_", "SYLPH_SPLIT_", "SYLPH_FUSE_")))


def _assert_forms(eng, kernels, routes, what):
    """The kernels that ran (profile records, in first-launch order) and the conv routes that were built (Engine.conv_routes(), in
    build order) are the ones the case names.  Not asserted under the routing overrides of the forced-variant reruns
    (tests/test_conv_variants_gpu.py), whose forms are the forced ones; the numbers are checked there all the same."""
    got_k, got_r = list(eng.profile_read()["kernels"]), eng.conv_routes()
    print(f"{what}: kernels {got_k}, conv routes {got_r}")
    if _routing_overrides():
        return
    assert got_k == kernels and got_r == routes, f"{what}: expected kernels {kernels} / routes {routes}, ran {got_k} / {got_r}"


def _assert_f32(got, want, what, rel=1e-4):
    got, want = got.float().cpu(), want.float().cpu()
    err = float((got - want).abs().max())
    scale = max(1.0, float(want.abs().max()))
    print(f"{what}: max |diff| {err:.3e} (scale {scale:.3f})")
    assert err <= rel * scale, f"{what}: max |diff| {err} > {rel} * {scale}"


# ------------------------------------------------------------------------------------------------ towers + prediction passes
TOWER_KERNELS = ["conv_hpipe_kernel<false>", "conv_hpipe_kernel<true>", "gn_taps_kernel+tap_gather_kernel", "gn_logits_kernel"]


def test_tower_and_prediction_kernels_pinned_on_full_pyramid():
    _tower_case(8)


def test_tower_and_prediction_kernels_pinned_at_batch1():
    _tower_case(1)


def _tower_case(B):
    """conv_hpipe<false> (first tower layer, GroupNorm statistics in the epilogue), conv_hpipe<true> (layers 2-4: the previous
    layer's GroupNorm + ReLU applied to the input halo in LDS), gn_logits_kernel, gn_taps_kernel + tap_gather_kernel: ONE
    launch each over all five levels of eight 800x1344 pyramids (per-level patch shapes, the pair list, ragged last patches;
    eight images so that the launch-size rule picks the same kernels as the B = 64 production step) -- and of ONE pyramid, the
    batch-1 query (SylphPredictor): 94 blocks per tower layer, still on conv_hpipe (the >= 90-block rule).
    Every layer is checked on the operands the HIP graph itself produced (its stored input + its coefficient table)."""
    from oracle import bf16 as OB16
    from oracle.head import HEAD_PREFIX
    from sylph_amd import synthetic as Wt
    N = 5
    sd = Wt.head_state_dict(seed=1, num_classes=60)
    g = torch.Generator().manual_seed(11)
    feats = [OB16.r(torch.randn(B, 256, h, w, generator=g)) for h, w in LEVELS]
    codes = Wt.synthetic_codes(N, seed=4, scale=3.0)
    eng = _engine("bf16", _cfg())
    eng.load_state_dict(sd)
    eng.set_debug_taps(True)
    eng.profile_enable(True)
    eng.import_pyramid(feats, (H, W))
    eng.head(codes["cls_conv"], codes["cls_bias"])
    _assert_forms(eng, TOWER_KERNELS, ["hpipe 256x256"] * 8, f"towers at batch {B}")
    eng.profile_enable(False)
    lo, rg, ct, io = eng.export_head()
    for t, name in ((0, "cls_tower"), (1, "bbox_tower")):
        x = feats
        for i in range(4):
            ys, cfs = eng.export_tower(t, i)
            nxt = []
            for l in range(5):
                v, y, cf = OB16.tower_layer(x[l], sd, f"{HEAD_PREFIX}.{name}", i)
                _assert_ulps(ys[l], y, f"{name} layer {i} level {l} (stored conv output)")
                _assert_f32(cfs[l], cf, f"{name} layer {i} level {l} (GroupNorm coefficients)")
                nxt.append(OB16.gn_apply(ys[l].cpu(), cfs[l].cpu()))  # the next layer's operand, from the HIP graph's own values
            x = nxt
        for l in range(5):
            if t == 0:
                _assert_f32(lo[l], OB16.cls_logits(x[l], codes["cls_conv"], codes["cls_bias"]), f"logits level {l}")
            else:
                reg, ctr, iou = OB16.predictions(x[l], sd, l)
                _assert_f32(rg[l], reg, f"reg level {l}")
                _assert_f32(ct[l], ctr, f"ctrness level {l}")
                _assert_f32(io[l], iou, f"iou level {l}")
    # many-way episode (LVIS-like, N > 32): the last cls-tower GroupNorm is applied in place (gn_apply_partials_kernel) and the
    # class-conditional conv runs on conv_igemm with fp32 output -- same operands, same bound
    ys, cfs = eng.export_tower(0, 3)
    ys, cfs = [t.cpu() for t in ys], [t.cpu() for t in cfs]
    many = Wt.synthetic_codes(337, seed=6, scale=2.0)
    eng.head(many["cls_conv"], many["cls_bias"])
    lo337 = eng.export_head()[0]
    for l in range(5):
        _assert_f32(lo337[l], OB16.cls_logits(OB16.gn_apply(ys[l], cfs[l]), many["cls_conv"], many["cls_bias"]), f"337-way logits level {l}")


# ------------------------------------------------------------------------------------------------ single backbone kernels
def _block_params(g, cin, mid, cout, shortcut):
    def conv(co, ci, k):
        return torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
    ws = [conv(mid, cin, 1), conv(mid, mid, 3), conv(cout, mid, 1)] + ([conv(cout, cin, 1)] if shortcut else [])
    scales = [0.5 + torch.rand(w.shape[0], generator=g) for w in ws]
    shifts = [0.2 * torch.randn(w.shape[0], generator=g) for w in ws]
    return ws, scales, shifts


I64, I128, IH, HP = "igemm 64x128 nbuf2", "igemm 128x128", "igemm_halo 128x128", "hpipe 256x256"
B1_64, B1_128, B1_128_2 = "igemm 64x64 nbuf3", "igemm 64x128 nbuf3", "igemm 64x128 nbuf2"
PW, PW2, SPW = "pw 128x256", "pw 256x128", "spw 128x256"
IG, RW3, SPWK, PWK = "conv_igemm_kernel", "conv_rw3_kernel", "conv_spw_kernel", "conv_pw_kernel"

BLOCKS = [
    # name, Cin, mid, cout, H, W, stride, shortcut, batch (large enough for the launch-size rules to pick the B = 64 kernels),
    # kernels that run (first-launch order), conv routes (conv1, conv2, conv3 [+ projection]; the fused / register-weight kernels
    # build no conv route)
    ("res2 identity (bottleneck64_kernel)", 256, 64, 256, 200, 336, 1, False, 2, ["bottleneck64_kernel"], []),
    ("res2 first block (bottleneck64p_kernel)", 64, 64, 256, 200, 336, 1, True, 2, ["bottleneck64p_kernel"], []),
    ("res3 identity", 512, 128, 512, 100, 168, 1, False, 4, [IG, RW3, SPWK], [I64, SPW]),
    ("res3 identity ragged map (partial last tiles on conv_igemm: no conv_rw3 patch fits 93 x 157, 457 M tiles < conv_spw's 512;"
     " the forced-variant reruns take it through both)", 512, 128, 512, 93, 157, 1, False, 4, [IG], [I64, I64, I128]),
    ("res3 first block (stride 2, conv3 + projection as one GEMM)", 256, 128, 512, 200, 336, 2, True, 4, [PWK, RW3], [PW2, PW]),
    ("res4 identity (conv2 on conv_hpipe)", 1024, 256, 1024, 50, 84, 1, False, 40, [PWK, "conv_hpipe_kernel<false>", SPWK], [PW, HP, SPW]),
    ("res5 first block", 1024, 512, 2048, 50, 84, 2, True, 16, [PWK, "conv_hpipe_kernel<false>"], [PW, HP, PW]),
    ("res5 identity", 2048, 512, 2048, 25, 42, 1, False, 32, [PWK, IG], [PW, IH, I128]),
]

# The batch-1 query (SylphPredictor, the reference's per-image query loop) at the map sizes of one 800 x 1333 image: the small-launch
# forms -- 64-row tiles, 64 x 64 tiles up to 160 64 x 128 tiles, three LDS stages up to 400 tiles.  (No block or lateral of one image
# splits K: their launches have more than 64 tiles; tests/test_conv_routes_gpu.py pins split K with and without a residual.)
BLOCKS_B1 = [
    ("res3 identity", 512, 128, 512, 100, 168, 1, False, 1, [IG], [B1_128, B1_128, B1_128_2]),
    ("res3 first block", 256, 128, 512, 200, 336, 2, True, 1, [IG, PWK], [B1_128, B1_128, PW]),
    ("res4 first block", 512, 256, 1024, 100, 168, 2, True, 1, [IG], [B1_64, B1_64, B1_128_2]),
    ("res4 identity", 1024, 256, 1024, 50, 84, 1, False, 1, [IG], [B1_64, B1_64, B1_128_2]),
    ("res5 first block", 1024, 512, 2048, 50, 84, 2, True, 1, [IG], [B1_64, B1_64, B1_128]),
    ("res5 identity", 2048, 512, 2048, 25, 42, 1, False, 1, [IG], [B1_64, B1_64, B1_128]),
]


def _run_block(case, what):
    from oracle import bf16 as OB16
    name, cin, mid, cout, h, w, stride, shortcut, B, kernels, routes = case
    g = torch.Generator().manual_seed(cin + mid)
    x = OB16.r(F.relu(torch.randn(B, cin, h, w, generator=g)))
    ws, scales, shifts = _block_params(g, cin, mid, cout, shortcut)
    eng = _engine("bf16")
    eng.profile_enable(True)
    y = eng.bottleneck(x, ws, scales, shifts, stride)
    _assert_forms(eng, kernels, routes, what)
    want = OB16.bottleneck(x, ws, scales, shifts, stride)
    _assert_ulps(y, want, what, max_ulp=2.0, max_frac=0.03, floor="rms")


@pytest.mark.parametrize("case", BLOCKS, ids=[c[0].split(" (")[0].replace(" ", "_") for c in BLOCKS])
def test_bottleneck_blocks_pinned_at_production_shape(case):
    """One bottleneck block of every stage at its 800x1344 map size through the launches the backbone uses for it (the fused
    res2 kernels, the pointwise / halo / hpipe conv kernels) against the bf16-storage oracle on the same input."""
    _run_block(case, case[0])


@pytest.mark.parametrize("case", BLOCKS_B1, ids=[c[0].replace(" ", "_") for c in BLOCKS_B1])
def test_bottleneck_blocks_pinned_at_batch1(case):
    """The same blocks as one 800x1333 query image takes them (res3-res5), on the batch-1 conv forms; the bound of one block."""
    _run_block(case, f"{case[0]} at batch 1")


LATERALS = [("fpn_lateral5", 2048, 25, 42, False, 32, PWK, PW), ("fpn_lateral4 (+ top-down)", 1024, 50, 84, True, 16, PWK, PW),
            ("fpn_lateral3 (+ top-down)", 512, 100, 168, True, 4, PWK, PW),
            # batch 1 (one 800 x 1333 query image): conv_igemm's small-launch forms, the top-down add in its epilogue
            ("fpn_lateral5 batch 1", 2048, 25, 42, False, 1, IG, B1_64), ("fpn_lateral4 batch 1 (+ top-down)", 1024, 50, 84, True, 1, IG, B1_64),
            ("fpn_lateral3 batch 1 (+ top-down)", 512, 100, 168, True, 1, IG, B1_128_2)]


@pytest.mark.parametrize("case", LATERALS, ids=[c[0].split(" (")[0].replace(" ", "_") for c in LATERALS])
def test_fpn_laterals_pinned_at_production_shape(case):
    """conv_pw_kernel<128, 256, 3, RES, false> on the FPN laterals: RES = 0 (lateral5) and RES = 2 (lateral4 / 3: the nearest-2x
    upsampled level above added as a residual in the epilogue) at their 800x1344 map sizes, batches large enough for the production
    kernel selection -- and at batch 1 on conv_igemm's small-launch forms; one conv, no bf16 intermediate: <= 1 ulp."""
    from oracle import bf16 as OB16
    name, cin, h, w, has_top, B, kernel, route = case
    g = torch.Generator().manual_seed(cin)
    x = OB16.r(F.relu(torch.randn(B, cin, h, w, generator=g)))
    wt = torch.randn(256, cin, 1, 1, generator=g) * (1.0 / cin) ** 0.5
    bias = 0.2 * torch.randn(256, generator=g)
    top = OB16.r(torch.randn(B, 256, h // 2, w // 2, generator=g)) if has_top else None
    eng = _engine("bf16")
    eng.profile_enable(True)
    y = eng.fpn_lateral(x, wt, bias, top)
    _assert_forms(eng, [kernel], [route], name)
    res = F.interpolate(top, scale_factor=2.0, mode="nearest") if has_top else None
    _, want = OB16.conv_epilogue(x, wt, None, bias, res_bf=res)
    _assert_ulps(y, want, name)


def test_stem_pool_kernel_pinned_at_800x1344():
    """stem_pool_kernel (7x7 s2 stem + FrozenBN + ReLU + 3x3 s2 max-pool in one pass) on two 800x1344 inputs."""
    from oracle import bf16 as OB16
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, H, W, generator=g) * 60.0
    w = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5 / 60.0
    scale, shift = 0.5 + torch.rand(64, generator=g), 0.2 * torch.randn(64, generator=g)
    eng = _engine("bf16")
    stem, pool = eng.stem_maxpool(x, w, scale, shift)
    _, ref_stem = OB16.conv_epilogue(OB16.r(x), w, scale, shift, stride=2, padding=3, relu=True)
    _assert_ulps(stem, ref_stem, "stem_conv_kernel")
    # the pool is exact on whatever stem values it sees: compare against the pool of the HIP stem for identity, and against
    # the oracle stem for the ulp bound of the fused kernel
    assert torch.equal(pool.cpu(), F.max_pool2d(stem.cpu(), 3, 2, 1)), "fused stem+pool differs from pooling the stand-alone stem output"
    _assert_ulps(pool, F.max_pool2d(ref_stem, 3, 2, 1), "stem_pool_kernel")


# ------------------------------------------------------------------------------------------------ whole backbone, stage by stage
@pytest.fixture(scope="module")
def full_sd():
    from sylph_amd import synthetic as Wt
    return Wt.synthetic_state_dict(0, depth=50)


def test_backbone_stagewise_pinned_at_800x1333(full_sd):
    """preprocess -> ResNet-50 -> FPN on one 800x1333 image (padded to 800x1344) in the production configuration; each stage
    output (sylph_export_stage) against the bf16-storage oracle started from the HIP graph's own previous stage, then the
    pyramid from the HIP graph's res3..res5.  Several chained blocks per stage: isolated flips spread (module docstring), so
    the bound is on the error energy (relative L2 <= 2^-8) and the worst element (16 ulps at the tensor's scale)."""
    from oracle import bf16 as OB16
    from sylph_amd import synthetic as Wt
    q = Wt.synthetic_images(1, 800, 1333, seed=3)
    eng = _engine("bf16", _cfg())
    eng.load_state_dict(full_sd)
    assert eng.preprocess(q) == (H, W)
    eng.backbone()
    x0 = eng.export_input().cpu()
    want_x0, _ = OB16.preprocess(q)
    assert torch.equal(x0, want_x0), "normalised bf16 network input differs"
    prev = None
    stages = {}
    for stage in (2, 3, 4, 5):
        got = eng.export_stage(stage).cpu()
        want = OB16.resnet(x0, full_sd, 50, start_stage=stage, x_stage=prev)[f"res{stage}"]
        _assert_chain(got, want, f"res{stage} (from the HIP graph's res{stage - 1})" if prev is not None else "stem + pool + res2")
        stages[f"res{stage}"] = got
        prev = got
    pyr = OB16.fpn(stages, full_sd)
    got_pyr = eng.export_pyramid()
    for l, k in enumerate(("p3", "p4", "p5", "p6", "p7")):
        _assert_chain(got_pyr[l], pyr[k], f"FPN {k} (from the HIP graph's res3..res5)")


# ------------------------------------------------------------------------------------------------ detections
def _cand_ordinals(inst, N):
    base, bases = 0, []
    for h, w in LEVELS:
        bases.append(base)
        base += h * w
    lv = inst["fpn_levels"].numpy()
    return (np.asarray(bases)[lv] + inst["loc_index"].numpy()) * N + inst["pred_classes"].numpy()


def test_detections_bf16_hip_vs_bf16_oracle_800x1333(full_sd):
    """End to end in the production mode against the bf16-storage oracle: the detections of an 800x1333 query must be the same
    (level, location, class) triples.  Residual differences are 1-ulp flips propagated through ~60 layers moving a score
    across the 0.05 threshold / an IoU across 0.6 / the top-100 cut (the synthetic-weight scores are densely packed around
    the cut): >= 90 % identical triples (measured 92-94 of 100 -- 93-94 with the kernel selection of rounds 4-5, 92 since the round-6
    small-launch changes: un-split K walks and 64 x 64 tiles sum the same products in another fp32 order; which near-ties flip is
    chance, what is NOT chance is checked next), scores of the common ones within 2e-2 (measured 1.0e-2) -- and every
    detection only one side reports is PROVED marginal on the head outputs of the side that lacks it (explain_absence): it fails
    exactly one decision, by at most 8e-3 on cls x quality (= score^2: the measured 1e-2 score spread of the COMMON detections at the
    score of the top-100 cut, 2 x 0.4 x 1e-2; measured margins 2.2e-3 ... 3.3e-3, all at the post-NMS top-100 cut) or 2e-2 on an IoU.
    The fp32-oracle comparison of the same path can only ask for class + IoU >= 0.9 on 90 % and 5e-2."""
    from oracle import bf16 as OB16
    from sylph_amd import synthetic as Wt
    q = Wt.synthetic_images(1, 800, 1333, seed=3)
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    eng = _engine("bf16", _cfg())
    eng.load_state_dict(full_sd)
    eng.preprocess(q)
    eng.backbone()
    eng.head(codes["cls_conv"], codes["cls_bias"])
    got = eng.decode()[0]
    hip_head = [[t.cpu() for t in ts] for ts in eng.export_head()]
    from oracle import decode as OD
    x, sizes = OB16.preprocess(q)
    ref_head = OB16.fcos_head(OB16.backbone_fpn(x, full_sd, 50), full_sd, codes)
    want = OD.detector_postprocess(OD.predict_proposals(*ref_head)[0], sizes[0], sizes[0][0], sizes[0][1])
    ref_ord, hip_ord = _cand_ordinals(want, 5), got["cand_index"].cpu().numpy()
    pos = {int(o): k for k, o in enumerate(hip_ord)}
    hit = np.array([o in pos for o in ref_ord.tolist()])
    print(f"bf16 HIP vs bf16 oracle: {hit.sum()} of {hit.size} detections are the same (level, location, class)")
    assert hit.size >= 50 and hit.mean() >= 0.90, hit.mean()
    from test_hip_parity import _keys_of_ordinals, _prove_residue
    _prove_residue(ref_head, _keys_of_ordinals(ref_ord, 800, 1344, 5), hip_head, _keys_of_ordinals(hip_ord, 800, 1344, 5), 0,
                   "bf16 HIP vs bf16 oracle", eps_val=8e-3, eps_iou=2e-2)
    sel = np.array([pos[int(o)] for o in ref_ord[hit].tolist()])
    ds = np.abs(got["scores"].cpu().numpy()[sel] - want["scores"].numpy()[hit]).max()
    print(f"max |dscore| over the common detections {ds:.5f}")
    assert ds <= 2e-2, ds
