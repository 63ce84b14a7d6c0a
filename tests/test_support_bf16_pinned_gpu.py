"""The support path (support images -> class codes) pinned stage by stage to bf16 ulps at the shapes production uses.

Each stage is checked on the operands the HIP graph itself produced (its exported input, Engine.export_support; the pyramid for the
first stage), against a float64 restatement of that stage rounded ONCE where the graph stores bf16 (oracle/bf16.py lists the storage
points).  Bounds, stated and not tuned (the derivations of tests/test_bf16_pinned_gpu.py and tests/test_conv_routes_gpu.py):
  * bf16 outputs of one kernel with no bf16 intermediate inside -- ROIAlign (fp32 sum of the bilinear samples / count), each
    GroupNorm layer's pre-GroupNorm conv output, the MS-CAM output: worst element <= 1 bf16 ulp (floor 1e-3 of the tensor maximum),
    <= 1 % of elements not identical.  ROIAlign's reference takes the sample coordinates in fp32, as the operator computes them
    for fp32 inputs (independent_refs.roi_pool_separable_f64 f32_coords): a coordinate rounded in float64 instead moves a sample by a
    few 1e-6 pixels, more than an ulp of a pooled value near the floor on a thin box.  A box wholly outside its level gives exact zeros.
  * GroupNorm (a, b) tables: fp32 from fp64 statistics, <= 1e-4 of max(1, max |want|).  The applied output, recomputed from the
    HIP y and table as bf16(act(fma(a, y, b))): identical.
  * fp32 outputs of a sum over K = 2304 ... 12544 products (cls / aux convs, the context pool, the token FCs and encoder layers,
    class tokens, code heads): <= 1e-4 of max(1, max |want|).  linear_kernel runs at S = 10, 60, 180 and 183 rows: one, four and twelve
    16-row groups, a partial last group at 10, 60 and 183.
  * codegen tail and normalize_codes: the per-element fp32 summation bound of tests/bf16_ulps.py codegen_tail_f64 (S * 49 additions per
    channel); normalised codes <= 1e-5 of their maximum (about 30 fp32 operations per element: 64 u).
  * end to end, from the HIP pyramid to the un-normalised code through the bf16 oracle: every stored stage can flip elements by an ulp
    and the flips move everything downstream, so the statement is the chain bound: relative L2 <= 2^-8, worst element <= 16 ulps at
    the rms floor (tests/bf16_ulps.py assert_chain); for every case and every class of a batch.
Batched-class independence: every class of a batched case gives the same stage outputs (within the bounds above: the conv route of
a one-class call can differ) and the same code as the same support images run alone.

Each case asserts the conv routes that ran (Engine.conv_routes()), except under the routing overrides of the forced-variant reruns.
The 7x7 ROI maps are one patch per image, so their routes depend only on the image count S: conv_igemm 64 x 64 tiles (three LDS
stages) up to 104 images for the tower and cls convs; conv_hpipe from 179 images ((S + 1) / 2 >= 90 blocks), where the flat pairing
puts two images' patches into one block and 183 images leave the pair list's empty pad patch.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bf16_ulps import assert_chain, assert_f32, assert_tail, assert_ulps, bf16_rne, codegen_tail_f64, conv_epilogue_f64
from independent_refs import level_of_box, roi_pool_separable_f64

pytestmark = pytest.mark.gpu

IG64, IG128, HP, AUX = "igemm 64x64 nbuf3", "igemm 64x128 nbuf3", "hpipe 256x256", "igemm 128x32"

# name, image size, classes, shots, route of the 7x7 tower convs, route of the cls conv (fp32 out: never hpipe)
CASES = [
    ("1x1 800x1344", (800, 1344), 1, 1, IG64, IG64),
    ("1x5 800x1344", (800, 1344), 1, 5, IG64, IG64),
    ("1x10 800x1344", (800, 1344), 1, 10, IG64, IG64),
    ("12x5 64x96", (64, 96), 12, 5, IG64, IG64),
    ("6x10 64x96", (64, 96), 6, 10, IG64, IG64),
    ("36x5 64x96", (64, 96), 36, 5, HP, IG128),
    ("61x3 64x96", (64, 96), 61, 3, HP, IG128),
]


def _routing_overrides():
    return sorted(k for k in os.environ if k.startswith(("SYLPH_CONV_", "SYLPH_SPLIT_", "SYLPH_FUSE_")))


def _expected_routes(S):
    """pick_conv_route for a 7x7 support conv of S images (csrc/api_conv.hip, conv_igemm.hip conv_pick_tile): rows = 49 S."""
    blocks_hp = (S + 1) // 2
    tower = HP if blocks_hp >= 90 else None
    bn = 64 if (49 * S + 63) // 64 * 2 <= 160 else 128
    igemm = f"igemm 64x{bn} nbuf{3 if S * (256 // bn) <= 400 else 2}"
    return tower or igemm, igemm


def test_case_table_reaches_every_route():
    """The table covers both sides of the hpipe threshold, the 64 x 128 cls-conv tiles, the pad patch of an odd pair list; a retuned
    threshold that moves a case off its route fails here by name."""
    for name, _, ncls, shots, tower, cls in CASES:
        assert _expected_routes(ncls * shots) == (tower, cls), name
    S = [n * s for _, _, n, s, _, _ in CASES]
    assert {c[4] for c in CASES} == {IG64, HP} and {c[5] for c in CASES} == {IG64, IG128}
    assert any(s % 2 == 1 and s >= 179 for s in S) and any(s % 2 == 0 and s >= 179 for s in S)
    assert max(s for s in S if s < 179) >= 60 and 10 in S and any(s > 16 and s % 16 for s in S)


def _cfg(roi_encoder=False, weight_scale=False):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    if weight_scale:
        cg.WEIGHT_LAYER = ["", "", 1]
        cg.SCALE_LAYER = ["", "", 1]
        cg.BIAS_L2_NORM = True
    if roi_encoder:
        cg.NAME = "ROIEncoder"
        cg.TOKENIZER.NUM_CONV, cg.TOKENIZER.CONV_DIM, cg.TOKENIZER.NORM = 2, 256, "GN"
        cg.TOKENIZER.NUM_FC, cg.TOKENIZER.FC_DIM = 2, 256
        cg.TRANSFORMER_ENCODER.LAYERS, cg.TRANSFORMER_ENCODER.HEADS = 2, 8
        cg.HEAD.NUM_FC, cg.HEAD.FC_DIM, cg.HEAD.OUTPUT_DIM = 2, 512, 256
    return cfg


def _state_dict(kind):
    from sylph_amd import synthetic as W
    if kind == "roienc":
        return W.roi_encoder_state_dict(seed=4)
    return W.codegen_state_dict(seed=2, weight_scale_layers=kind == "weighted")


GENERATORS = ["codegen", "roienc"]


def _engine(kind, dtype="bf16", taps=True):
    from sylph_amd.engine import Engine
    eng = Engine(_cfg(kind == "roienc", kind == "weighted"), dtype=dtype)
    eng.load_state_dict(_state_dict(kind))
    eng.set_debug_taps(taps)
    eng.profile_enable(True)
    return eng


# ------------------------------------------------------------------------------------------------ inputs
def _pyramid(S, H, W, seed):
    from oracle import bf16 as OB16
    g = torch.Generator().manual_seed(seed)
    shapes = []
    h, w = H // 8, W // 8
    for _ in range(5):
        shapes.append((h, w))
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return [OB16.r(torch.randn(S, 256, h, w, generator=g)) for h, w in shapes]


def _box_kinds(H, W):
    """Boxes (xyxy image pixels) that reach every FPN level 3..7 and the edges of ROIAlign: sqrt(area) exactly at 224 * 2^k (the
    boundary belongs to the upper level, in fp32 and float64 alike), boxes straddling each image border, boxes wholly outside the
    image (far enough that every sample of their level is outside [-1, size]: exact zeros), thin boxes (one sample per bin)."""
    s = min(H, W) / 800.0
    cx, cy = W / 2, H / 2
    kinds = []
    for bw, bh in ((112, 112), (224, 224), (448, 448), (1024, 784), (1792, 1792)):  # levels 3, 4, 5, 6, 7
        kinds.append((cx - bw / 2 + 0.25, cy - bh / 2, cx + bw / 2 + 0.25, cy + bh / 2))
    d = max(8.0, 60 * s)
    kinds += [(-d, cy - 2 * d, d, cy + d), (cx - d, -1.5 * d, cx + 2 * d, d), (W - d, cy, W + 1.5 * d, cy + 2 * d),
              (cx, H - d, cx + 3 * d, H + d)]  # straddling left, top, right, bottom
    kinds += [(W + 300.0, 10.0, W + 400.0, 110.0), (-400.0, H + 300.0, -300.0, H + 380.0)]  # wholly outside (level 3)
    kinds += [(cx, cy - 150 * s, cx + 2.0, cy + 150 * s), (10.0, cy, 10.0 + 400 * s, cy + 1.5)]  # thin
    return torch.tensor(kinds, dtype=torch.float32)


def _box_sets(S, H, W, seed):
    """Box lists of S boxes each such that every kind of _box_kinds appears in the case (one call per list), the rest random."""
    kinds = _box_kinds(H, W)
    g = torch.Generator().manual_seed(seed)
    sets = []
    for j in range((len(kinds) + S - 1) // S):
        b = kinds[j * S:(j + 1) * S]
        n = S - b.shape[0]
        if n:
            x0 = torch.rand(n, generator=g) * 0.8 * W
            y0 = torch.rand(n, generator=g) * 0.8 * H
            bw = 8 + torch.rand(n, generator=g) * 0.6 * W
            bh = 8 + torch.rand(n, generator=g) * 0.6 * H
            b = torch.cat([b, torch.stack([x0, y0, x0 + bw, y0 + bh], dim=1)])
        sets.append(b[torch.randperm(S, generator=g)])
    return sets


def _outside(box, H, W):
    return box[0] > W + 200 or box[2] < -200 or box[1] > H + 200 or box[3] < -200


# ------------------------------------------------------------------------------------------------ stage checks
def _f64(sd, keys_prefix):
    return {k: v.double() for k, v in sd.items() if k.startswith(keys_prefix)}


def _check_roi(eng, pyr, boxes, H, W, what):
    got = eng.export_support("roi").cpu()
    want = bf16_rne(torch.from_numpy(roi_pool_separable_f64([p.numpy() for p in pyr], boxes.numpy(), f32_coords=True)))
    assert_ulps(got, want, f"{what} ROIAlign")
    lv = [level_of_box(b.tolist()) for b in boxes]
    for i, b in enumerate(boxes):
        if _outside(b.tolist(), H, W):
            assert float(got[i].abs().max()) == 0.0, f"{what}: box {i} lies outside the image, ROIAlign must give zeros"
    return got, sorted(set(lv))


def _conv_f64(x, w, b):
    """fp32-output support conv in float64: bf16 operands (the HIP input as given, bf16 weights) + bias."""
    from oracle import bf16 as OB16
    return F.conv2d(x.double(), OB16.r(w).double(), None, padding=1) + b.double().view(1, -1, 1, 1)


def _check_gn_layer(eng, x, w, b, gamma, beta, index, act_relu, what):
    """One GroupNorm layer on the HIP graph's own input x: pre-GroupNorm output, (a, b) table, applied output."""
    from oracle import bf16 as OB16
    y = eng.export_support("gn_y", index).cpu()
    cf = eng.export_support("gn_coef", index).cpu()
    out = eng.export_support("layer_out", index).cpu()
    shift = b if b is not None else torch.zeros(w.shape[0])
    v = conv_epilogue_f64(x, OB16.r(w), torch.ones(w.shape[0]), shift, 1, 1)
    assert_ulps(y, bf16_rne(v), f"{what} layer {index} stored pre-GroupNorm output")
    assert_f32(cf, OB16.gn_coef(v, gamma, beta), f"{what} layer {index} GroupNorm coefficients")
    assert torch.equal(out, OB16.gn_apply(y, cf, act_relu)), f"{what} layer {index}: applied output is not bf16(act(fma(a, y, b)))"
    return y, cf, out


def _check_codegen(eng, kind, sd, pyr, boxes, shots, codes, H, W, what):
    from oracle import bf16 as OB16
    from oracle.codegen import CG_PREFIX
    roi, levels = _check_roi(eng, pyr, boxes, H, W, what)
    x = roi
    p = f"{CG_PREFIX}.support_set_shared_tower"
    for i in range(2):
        x = _check_gn_layer(eng, x, sd[f"{p}.{3 * i}.weight"], sd[f"{p}.{3 * i}.bias"], sd[f"{p}.{3 * i + 1}.weight"],
                            sd[f"{p}.{3 * i + 1}.bias"], i, True, what)[2]
    conv = eng.export_support("conv_out", 0).cpu()
    aux = eng.export_support("conv_out", 1).cpu()
    names = ["support_set_cls_bias"] + (["support_set_cls_weight", "support_set_cls_scale"] if kind == "weighted" else [])
    assert_f32(conv, _conv_f64(x, sd[f"{CG_PREFIX}.support_set_cls_conv.0.weight"], sd[f"{CG_PREFIX}.support_set_cls_conv.0.bias"]),
               f"{what} cls conv")
    assert aux.shape[1] == len(names)
    for j, n in enumerate(names):
        assert_f32(aux[:, j:j + 1], _conv_f64(x, sd[f"{CG_PREFIX}.{n}.0.weight"], sd[f"{CG_PREFIX}.{n}.0.bias"]), f"{what} {n} conv")
    weighted = kind == "weighted"
    want, wn, tol = codegen_tail_f64(conv, aux[:, 0:1], shots, aux[:, 1:2] if weighted else None, aux[:, 2:3] if weighted else None,
                                     bias_l2_norm=weighted)
    assert_tail(codes.cpu(), want, tol, f"{what} codegen tail")
    if weighted:
        wn_got = eng.codegen_weight_norm(codes.shape[0]).cpu()
        assert float((wn_got.double() - wn).abs().max()) <= 1e-5 * max(1.0, float(wn.abs().max())), f"{what} cls_weight_norm"
        _check_normalize(eng, sd, codes, wn_got, what)
    else:
        _check_normalize(eng, sd, codes, None, what)
    return levels


def _check_normalize(eng, sd, codes, wn, what):
    from oracle.codegen import normalize_code
    got = eng.normalize_codes(codes.clone().contiguous(), wn).cpu()
    sd64 = {k: v.double() for k, v in sd.items()}
    for k in range(codes.shape[0]):
        c, b = normalize_code(codes[k, :256].cpu().double().view(1, 256, 1, 1), codes[k, 256:].cpu().double().view(1, 1, 1, 1), sd64,
                              cls_weight_norm=None if wn is None else wn[k].double())
        want = torch.cat([c.reshape(-1), b.reshape(-1).double()])
        err = float((got[k].double() - want).abs().max())
        assert err <= 1e-5 * float(want.abs().max()), f"{what} normalize_codes class {k}: {err}"


def _check_roienc(eng, sd, pyr, boxes, shots, codes, H, W, what):
    from oracle import bf16 as OB16
    from oracle import roi_encoder as R
    roi, levels = _check_roi(eng, pyr, boxes, H, W, what)
    ctx = eng.export_support("context").cpu()
    assert_f32(ctx, OB16.roienc_context([p.double() for p in pyr]), f"{what} context")
    bp = "code_generator.box_pooler.conv"
    x0 = _check_gn_layer(eng, roi, sd[f"{bp}.0.weight"], sd[f"{bp}.0.bias"], sd[f"{bp}.1.weight"], sd[f"{bp}.1.bias"], 0, True, what)[2]
    cam = eng.export_support("mscam").cpu()
    sd64 = {k: v.double() for k, v in sd.items()}
    assert_ulps(cam, bf16_rne(R.ms_cam(x0.double(), ctx.double(), sd64, "code_generator.box_pooler.context_attention_module")),
                f"{what} MS-CAM output")
    x = cam
    for k in range(2):
        t = f"code_generator.tokenizer.conv{k + 1}"
        x = _check_gn_layer(eng, x, sd[f"{t}.weight"], None, sd[f"{t}.norm.weight"], sd[f"{t}.norm.bias"], 1 + k, True, what)[2]
    tok = eng.export_support("tokens", 0).cpu()
    assert_f32(tok, OB16.tokenizer_fc(x.double(), sd64), f"{what} tokens after the FC stack ({tok.shape[0]} rows)")
    for l in range(2):
        nxt = eng.export_support("tokens", l + 1).cpu()
        assert_f32(nxt, R.encoder_layer(tok.double().unsqueeze(0), sd64, f"code_generator.transformer_encoder.layers.{l}", 8)[0],
                   f"{what} tokens after encoder layer {l}")
        tok = nxt
    cls = eng.export_support("cls_tokens").cpu()
    assert_f32(cls, tok.double().view(-1, shots, 256).mean(dim=1), f"{what} class tokens")
    assert_f32(codes.cpu(), OB16.roienc_heads(cls.double(), sd64), f"{what} code heads")
    return levels


def _oracle_codes(kind, sd, pyr, boxes, shots):
    from oracle import bf16 as OB16
    if kind == "roienc":
        return OB16.roi_encoder_support(pyr, boxes, sd, shots)["codes"]
    w = kind == "weighted"
    return OB16.codegen_support(pyr, boxes, sd, shots, weight_layer=w, scale_layer=w, bias_l2_norm=w)["codes"]


def _check_end_to_end(codes, want, what):
    for k in range(codes.shape[0]):
        assert_chain(codes[k, :256].cpu(), want[k, :256], f"{what} class {k} code")
        b, bw = float(codes[k, 256]), float(want[k, 256])
        assert abs(b - bw) <= 2.0 ** -8 * max(1.0, abs(bw)), f"{what} class {k} bias {b} vs {bw}"


def _run(eng, pyr, hw, boxes, shots):
    eng.import_pyramid(pyr, hw)
    return eng.codegen_classes(boxes, shots).clone()


@pytest.mark.parametrize("kind", GENERATORS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_support_path_pinned(case, kind):
    _pinned(case, kind)


WEIGHTED_CASES = [CASES[1], CASES[3], CASES[6]]


@pytest.mark.parametrize("case", WEIGHTED_CASES, ids=[c[0] for c in WEIGHTED_CASES])
def test_weighted_code_generator_pinned(case):
    """WEIGHT_LAYER (softmax shot weights), SCALE_LAYER (cls_weight_norm) and BIAS_L2_NORM: the three 1-channel heads as one stacked
    conv, the weighted pools of codegen_tail_kernel, normalize_codes with the weight norm."""
    _pinned(case, "weighted")


def _pinned(case, kind):
    name, (H, W), ncls, shots, tower, cls = case
    S = ncls * shots
    sd = _state_dict(kind)
    pyr = _pyramid(S, H, W, seed=S)
    eng = _engine(kind)
    seen = set()
    for j, boxes in enumerate(_box_sets(S, H, W, seed=100 + S)):
        what = f"{name} {kind} call {j}"
        codes = _run(eng, pyr, (H, W), boxes, shots)
        if j == 0:
            routes = eng.conv_routes()
            want = [tower] * 3 if kind == "roienc" else [tower, tower, cls, AUX]
            print(f"{what}: conv routes {routes}")
            if not _routing_overrides():
                assert routes == want, f"{what}: expected routes {want}, ran {routes}"
        hp = eng.export_pyramid()
        assert all(torch.equal(a.cpu(), b) for a, b in zip(hp, pyr)), "the imported pyramid is bf16: it must come back unchanged"
        if kind == "roienc":
            seen |= set(_check_roienc(eng, sd, pyr, boxes, shots, codes, H, W, what))
        else:
            seen |= set(_check_codegen(eng, kind, sd, pyr, boxes, shots, codes, H, W, what))
        _check_end_to_end(codes, _oracle_codes(kind, sd, pyr, boxes, shots), what)
    assert seen == {3, 4, 5, 6, 7}, f"{name}: boxes reached levels {sorted(seen)}"


@pytest.mark.parametrize("kind", GENERATORS)
@pytest.mark.parametrize("case", [c for c in CASES if c[2] > 1], ids=[c[0] for c in CASES if c[2] > 1])
def test_batched_classes_equal_one_class_per_call(case, kind):
    """Every class of a batched call: the stage outputs and the code of the same support images run alone (codegen)."""
    name, (H, W), ncls, shots, _, _ = case
    S = ncls * shots
    pyr = _pyramid(S, H, W, seed=S)
    boxes = _box_sets(S, H, W, seed=100 + S)[0]
    batched = _engine(kind)
    codes = _run(batched, pyr, (H, W), boxes, shots)
    # one kernel on the same operands: the ulp bound; stages behind a stored bf16 stage of the other run (whose flips they inherit):
    # the chain bound
    direct = [("roi", 0), ("gn_y", 0)]
    chained = [("gn_y", 1), ("layer_out", 1)] + ([("mscam", 0), ("gn_y", 2), ("tokens", 0), ("tokens", 2)] if kind == "roienc"
                                                 else [("conv_out", 0)])
    got = {s: batched.export_support(*s).cpu() for s in direct + chained}
    single = _engine(kind)
    for k in range(ncls):
        sl = slice(k * shots, (k + 1) * shots)
        one = _run(single, [p[sl] for p in pyr], (H, W), boxes[sl], shots)
        for s in direct + chained:
            mine = single.export_support(*s).cpu()
            (assert_ulps if s in direct else assert_chain)(got[s][sl], mine, f"{name} {kind} class {k} {s[0]} {s[1]}")
        assert_chain(codes[k, :256].cpu(), one[0, :256].cpu(), f"{name} {kind} class {k} code")
        assert abs(float(codes[k, 256]) - float(one[0, 256])) <= 2.0 ** -8 * max(1.0, abs(float(one[0, 256])))


def test_taps_change_no_kernel():
    """Debug taps copy stages aside; the kernels, their routes and the codes are the same with and without them."""
    name, (H, W), ncls, shots, _, _ = CASES[3]
    S = ncls * shots
    pyr = _pyramid(S, H, W, seed=S)
    boxes = _box_sets(S, H, W, seed=100 + S)[0]
    for kind in GENERATORS:
        runs = []
        for taps in (False, True):
            eng = _engine(kind, taps=taps)
            codes = _run(eng, pyr, (H, W), boxes, shots)
            runs.append((eng.conv_routes(), list(eng.profile_read()["kernels"]), codes.cpu()))
        print(f"{kind}: routes {runs[0][0]}, kernels {runs[0][1]}")
        assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1], f"{kind}: taps changed the kernels"
        assert torch.equal(runs[0][2], runs[1][2]), f"{kind}: taps changed the codes"


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_fp32_modes_match_fp32_oracle_12x5(dtype):
    """The fp32 and split-bf16 modes at the benchmark's 60-image batch: codes within 1e-3 of the fp32 oracle (the statement of the
    golden tests at <= 5 images)."""
    from oracle import codegen as CG, roi_encoder as R
    name, (H, W), ncls, shots, _, _ = CASES[3]
    S = ncls * shots
    pyr = _pyramid(S, H, W, seed=S)
    boxes = _box_sets(S, H, W, seed=100 + S)[0]
    for kind in GENERATORS:
        sd = _state_dict(kind)
        codes = _run(_engine(kind, dtype=dtype, taps=False), pyr, (H, W), boxes, shots).cpu()
        for k in range(ncls):
            sl = slice(k * shots, (k + 1) * shots)
            if kind == "roienc":
                ref = R.roi_encoder([p[sl] for p in pyr], boxes[sl], sd, num_shots=shots)
            else:
                ref = CG.code_generator([p[sl] for p in pyr], boxes[sl], sd)
            want = torch.cat([ref["cls_conv"].reshape(-1), ref["cls_bias"].reshape(-1)])
            err = float((codes[k] - want).abs().max())
            print(f"{dtype} {kind} class {k}: max |diff| {err:.2e}")
            assert err <= 1e-3 * max(1.0, float(want.abs().max())), (dtype, kind, k, err)
