"""Query steps in flight (Engine.decode_launch / Engine.decode_fetch; C ABI underneath: sylph_preprocess, sylph_preprocess_u8,
sylph_import_pyramid, sylph_fcos_head, sylph_fcos_head_codesets, sylph_import_head, sylph_decode_nms, sylph_decode_nms_codesets).

The serving loop of INTEGRATION.md (section E) and the benchmark enqueue `preprocess -> backbone -> head -> decode_launch` of step
k + 1 before `decode_fetch` reads step k back.  Every other GPU test reads a step back before it enqueues the next one, so the host
state that only matters while steps overlap is pinned here and nowhere else: the pinned staging tables that are rewritten per call
behind one event each (Plan::img_desc_host, Plan::rz_host, Plan::img_out_host), the "table unchanged: no upload" shortcut next to
them, buffers that grow between steps (candidate buffers, resize table), the pinned count buffers of the handles, and the engine
following torch's current stream.

Every test drives ONE engine through a list of steps with nothing read back until the whole list is enqueued, and compares every
step, field for field and bit for bit (torch.equal; no tolerance anywhere in this file), with
  * a second engine (same weights, same dtype) driven through the same list synchronously: decode(), then torch.cuda.synchronize(),
    after every step; and, for the first and the last step of a queue,
  * a fresh engine that ran only that step (the premise of test_call_sequences_gpu.py: identical kernels on identical inputs are
    deterministic);
and one step per test goes through the oracle decoder on that step's exported head outputs, so that the engines cannot all be wrong
in the same way.  A reference must find detections, and steps that a mix-up could confuse (neighbours; steps j and j + 8, the old
period of the count buffers) must differ in their references: otherwise the queue proves nothing, and the test says so.
The tests keep every input tensor (pyramids, images, codes) alive until after the last fetch: the library's state is under test,
not the caller's tensor lifetimes.

The steps: scenarios 1, 3 and 4 enqueue import_pyramid (plan A 128x160, plan B 96x128: the golden pyramid) -> head -> decode_launch;
scenarios 2, 5 and 6 enqueue preprocess / preprocess_u8 -> backbone -> head -> decode_launch on synthetic images of at most 128x160 (R-18 weights: _full_cfg).
bf16 throughout (the fused many-way scan exists only there); the first queue also in fp32."""
import pytest
import torch

from test_call_sequences_gpu import (FIELDS, PAD_A, PAD_B, _assert_oracle, _assert_same, _head, _pyr_b, _sizes, _thin,
                                     g1, sd)  # noqa: F401  (g1, sd: fixtures)
from test_hip_parity import _cfg, _engine, _feats

pytestmark = pytest.mark.gpu

_SHARED = {}  # references (CPU tensors, never modified) shared between the tests of this module


def _shared(key, make):
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def _cpu(dets):
    return [{k: d[k].cpu() for k in FIELDS} for d in dets]


def _counts(dets):
    return [int(d["scores"].numel()) for d in dets]


def _differ(a, b):
    """Two reference results that a mix-up would not leave unnoticed: another count on some image, or other scores."""
    return _counts(a) != _counts(b) or any(not torch.equal(x["scores"], y["scores"]) for x, y in zip(a, b))


def _assert_step(got, want, what, ref="the synchronous engine"):
    """got (device or host dicts) == want (host dicts), exactly; the message names the step and the field."""
    got = _cpu(got)
    assert len(got) == len(want), f"{what}: {len(got)} result slots, {len(want)} from {ref}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["scores"].numel() == w["scores"].numel(), \
            f"{what}: image {i}: detection count: {g['scores'].numel()} in flight, {w['scores'].numel()} from {ref}"
        for k in FIELDS:
            assert torch.equal(g[k], w[k]), f"{what}: image {i}: {k} differs from {ref}'s"


def _assert_non_vacuous(refs, pairs, what):
    for j, r in enumerate(refs):
        if r is not None:
            print(f"{what}: step {j}: detections per slot {_counts(r)}")
            assert sum(_counts(r)) > 0, f"{what}: step {j} decodes nothing on the synchronous engine -- the queue proves nothing"
    for a, b in pairs:
        if refs[a] is not None and refs[b] is not None:
            assert _differ(refs[a], refs[b]), f"{what}: steps {a} and {b} have the same reference -- a mix-up of the two would go unnoticed"


def _neighbours(n):
    return [(j, j + 1) for j in range(n - 1)] + [(j, j + 8) for j in range(n - 8)]


def _mk(dtype, weights, cfg=None, **kw):
    eng = _engine(dtype, cfg if cfg is not None else _cfg(), **kw)
    eng.load_state_dict(weights)
    return eng


def _run_sync(eng, steps, inp, enqueue):
    """The reference protocol: every step decoded and read back, and the device idle, before the next one is enqueued.  -> host dicts
    per step (None for a step whose decode raises as the step says it must)."""
    out = []
    for st in steps:
        enqueue(eng, st, inp, True)
        if st.get("raises"):
            with pytest.raises(RuntimeError, match=st["raises"]):
                eng.decode(st.get("out"), st.get("max_out"))
            out.append(None)
        else:
            out.append(_cpu(eng.decode(st.get("out"), st.get("max_out"))))
        torch.cuda.synchronize()
    return out


def _run_queued(eng, steps, inp, enqueue):
    """Every step enqueued, none read back.  -> the handles."""
    handles = []
    for st in steps:
        enqueue(eng, st, inp, False)
        handles.append(eng.decode_launch(st.get("out"), st.get("max_out")))
    return handles


def _sync_reference(dtype, weights, steps, inp, enqueue, cfg=None, **kw):
    eng = _mk(dtype, weights, cfg, **kw)
    out = _run_sync(eng, steps, inp, enqueue)
    eng.close()
    return out


def _fresh_steps(dtype, weights, steps, make_inp, enqueue, what, got, oracle=None, cfg=None, share=None, **kw):
    """The first and the last step of a queue, each alone on a fresh engine, == what the queue returned for them (got: host dicts per
    step); `oracle` = (step, threshold, head outputs or None): that step must be the first or the last, and its detections == the oracle
    decoder on the given head outputs (None: on those the fresh engine exports).  `share` names the engine setup (weights, dtype, config)
    of queues that have steps in common: a fresh engine's result for such a step is computed once per module."""
    assert oracle is None or oracle[0] in (0, len(steps) - 1)
    for j in sorted({0, len(steps) - 1}):
        export = oracle is not None and oracle[0] == j and oracle[2] is None
        before = tuple(steps[k]["overwrite"] for k in range(j) if "overwrite" in steps[k])
        key = ("fresh", share, dtype, tuple(sorted(steps[j].items())), before)
        hit = _SHARED.get(key) if share is not None else None
        if hit is None or (export and hit[1] is None):
            inp = make_inp()
            for k in range(j):  # in-place writes of earlier steps into tensors this step reads are part of its input
                if "overwrite" in steps[k]:
                    _overwrite(inp, steps[k])
            eng = _mk(dtype, weights, cfg, **kw)
            enqueue(eng, steps[j], inp, True)
            want = _cpu(eng.decode(steps[j].get("out"), steps[j].get("max_out")))
            heads = [[t.cpu() for t in ts] for ts in eng.export_head()] if export else None
            hit = (want, heads, list(eng._batch[3]))
            eng.close()
            if share is not None:
                _SHARED[key] = hit
        _assert_same(got[j], hit[0], f"{what}: step {j}")
        if oracle is not None and oracle[0] == j:
            assert steps[j].get("out") is None
            _assert_oracle(got[j], oracle[2] if oracle[2] is not None else hit[1], hit[2], thr=oracle[1])


# ================================================================================================ head + decode steps (scenarios 1, 3, 4)
class _HeadInputs:
    """Device-resident inputs of the head + decode steps (no host-to-device copy, hence no hidden wait, inside a queue)."""

    def __init__(self, g1, heads=None):
        from sylph_amd import synthetic as W
        dev = torch.device("cuda", 0)
        self.pyr = {"A": [t.to(dev).contiguous() for t in _feats(g1)], "B": [t.to(dev).contiguous() for t in _pyr_b(g1)]}
        self.sizes = _sizes(g1)
        self.codes = {"few": {"cls_conv": torch.from_numpy(g1["n5_t50_cls_conv"]).to(dev), "cls_bias": torch.from_numpy(g1["n5_t50_cls_bias"]).to(dev)},
                      "many": {k: v.to(dev) for k, v in W.synthetic_codes(60, seed=77, scale=3.0).items()},  # 60-way: the fused scan in bf16
                      "c20": {k: v.to(dev) for k, v in W.synthetic_codes(20, seed=50, scale=2.5).items()}}
        for j, (n, scale) in enumerate(DEEP_CODES):
            self.codes[f"d{j}"] = {k: v.to(dev) for k, v in W.synthetic_codes(n, seed=300 + n, scale=scale).items()}
        self.heads = heads or {}
        torch.cuda.synchronize()


def _enqueue_head(eng, st, inp, sync):
    """import_pyramid -> head (or import_head; or head_code_sets) of one step.  On the synchronous engine the head call also asserts
    which scan ran (profile_read waits for the stream, so not in a queue)."""
    if st["plan"] == "A":
        eng.import_pyramid(inp.pyr["A"], PAD_A, inp.sizes)
    else:
        eng.import_pyramid(inp.pyr["B"], PAD_B)
    if "heads" in st:
        eng.import_head(*inp.heads[st["heads"]])
    elif "sets" in st:
        eng.head_code_sets([(inp.codes[c]["cls_conv"], inp.codes[c]["cls_bias"]) for c in st["sets"]])
    else:
        c = inp.codes[st["codes"]]
        if sync:
            _head(eng, c, eng.dtype == "bf16" and c["cls_conv"].shape[0] > 32)
        else:
            eng.head(c["cls_conv"], c["cls_bias"])


# plan A: image sizes (128, 153), (123, 160); plan B: (96, 128) twice.  out None: the image sizes themselves
OUT_A1, OUT_A2 = [(256, 306), (200, 260)], [(96, 115), (150, 195)]
OUT_B1, OUT_B2 = [(192, 256), (120, 160)], [(77, 101), (144, 192)]
# Consecutive steps differ in plan, class codes (5-way plain scan, 60-way fused scan in bf16, 20-way: the candidate capacity of plan A
# grows twice in the queue, and on plan B a plain scan follows a fused one whose decode no one has read), out_sizes (plan A: None, then
# two different rescales, so img_out_host is rewritten while the plan's previous decode is queued) and max_out (None = 200).
QUEUE_1 = [dict(plan="A", codes="few", out=None, max_out=None),
           dict(plan="B", codes="many", out=OUT_B1, max_out=150),
           dict(plan="A", codes="c20", out=OUT_A1, max_out=120),
           dict(plan="B", codes="few", out=None, max_out=None),
           dict(plan="A", codes="many", out=OUT_A2, max_out=130),
           dict(plan="B", codes="c20", out=OUT_B2, max_out=110)]


@pytest.mark.parametrize("order", ["in order", "reversed"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_head_decode_queue_six_in_flight(g1, sd, dtype, order):
    """Scenario 1: six import -> head -> decode_launch steps in flight (QUEUE_1), fetched in order or last first."""
    what = f"head + decode queue ({dtype})"
    inp = _HeadInputs(g1)
    refs = _shared(("queue 1", dtype), lambda: _sync_reference(dtype, sd, QUEUE_1, inp, _enqueue_head))
    _assert_non_vacuous(refs, _neighbours(len(QUEUE_1)) + [(2, 4), (1, 3), (3, 5)], what)  # (also: the same plan's next step)
    eng = _mk(dtype, sd)
    handles = _run_queued(eng, QUEUE_1, inp, _enqueue_head)
    idx = list(range(len(handles)))
    got = {}
    for j in (idx if order == "in order" else idx[::-1]):
        got[j] = _cpu(eng.decode_fetch(handles[j]))
        _assert_step(got[j], refs[j], f"{what}, fetched {order}: step {j} of {len(handles)} in flight")
    eng.close()
    _fresh_steps(dtype, sd, QUEUE_1, lambda: inp, _enqueue_head, what, got, oracle=(0, 0.05, None))


# ------------------------------------------------------------------------------------------------ the deep queue
# (classes, code scale) of step j (synthetic_codes, seed 300 + classes): plain scans and three fused ones (more than 32 classes).  Most
# code sets fill the 100 detections per image of POST_NMS_TOPK_TEST; the small scales are there because steps j and j + 8 must differ
# in their COUNTS (a handle that reads another step's count buffer then returns rows cut at the wrong length).
DEEP_CODES = [(5, 1.5), (3, 1.75), (60, 2.5), (9, 1.5), (33, 2.0), (4, 1.25), (20, 1.0), (1, 2.5), (3, 1.5), (40, 2.5), (4, 1.5), (5, 1.25)]
QUEUE_DEEP = [dict(plan="A", codes=f"d{j}") for j in range(len(DEEP_CODES))]


def _deep_refs(g1, sd, inp):
    refs = _shared("deep", lambda: _sync_reference("bf16", sd, QUEUE_DEEP, inp, _enqueue_head))
    _assert_non_vacuous(refs, _neighbours(len(QUEUE_DEEP)), "deep queue")
    for j in range(len(refs) - 8):
        assert _counts(refs[j]) != _counts(refs[j + 8]), f"deep queue: steps {j} and {j + 8} have the same counts {_counts(refs[j])}"
    return refs


def test_deep_queue_twelve_in_flight(g1, sd):
    """Scenario 3: twelve decode_launch handles of one batch size outstanding before the first fetch: every handle returns its own step's
    detections (its own counts and its own status word), however many decodes were launched after it."""
    inp = _HeadInputs(g1)
    refs = _deep_refs(g1, sd, inp)
    eng = _mk("bf16", sd)
    handles = _run_queued(eng, QUEUE_DEEP, inp, _enqueue_head)
    got = {}
    for j, h in enumerate(handles):
        got[j] = _cpu(eng.decode_fetch(h))
        _assert_step(got[j], refs[j], f"deep queue: step {j} of {len(handles)} in flight")
    with pytest.raises(RuntimeError, match="fetched already"):
        eng.decode_fetch(handles[0])
    # the steady serving loop allocates no pinned buffer after warm-up: twelve in flight made twelve, two in flight reuse two of them
    pool = {id(b) for b in eng._counts_free[3]}
    assert len(pool) == len(handles) and not eng._counts_out
    pend = []
    for st in QUEUE_DEEP[:6]:
        pend.append(_run_queued(eng, [st], inp, _enqueue_head)[0])
        if len(pend) >= 2:
            eng.decode_fetch(pend.pop(0))
    eng.decode_fetch(pend.pop(0))
    assert {id(b) for b in eng._counts_free[3]} == pool and not eng._counts_out
    eng.close()
    _fresh_steps("bf16", sd, QUEUE_DEEP, lambda: inp, _enqueue_head, "deep queue", got, oracle=(0, 0.05, None))


def test_one_handle_outstanding_over_eight_synchronous_decodes(g1, sd):
    """Scenario 3, first variant: one handle outstanding, eight synchronous decode() calls of the same batch size, then the fetch of the first handle."""
    inp = _HeadInputs(g1)
    refs = _deep_refs(g1, sd, inp)
    eng = _mk("bf16", sd)
    first = _run_queued(eng, QUEUE_DEEP[:1], inp, _enqueue_head)[0]
    for j in range(1, 9):
        _enqueue_head(eng, QUEUE_DEEP[j], inp, False)
        _assert_step(eng.decode(), refs[j], f"synchronous decode {j} behind an outstanding handle")
    got = _cpu(eng.decode_fetch(first))
    _assert_step(got, refs[0], "step 0, fetched after eight synchronous decodes")
    eng.close()
    fresh = _mk("bf16", sd)
    _enqueue_head(fresh, QUEUE_DEEP[0], inp, True)
    _assert_same(got, _cpu(fresh.decode()), "step 0, fetched after eight synchronous decodes")
    _assert_oracle(got, fresh.export_head(), inp.sizes)
    fresh.close()


# step 0: a decode_launch handle of the plain path; steps 1-9: head_code_sets + decode_code_sets (synchronous) of one or two code sets
QUEUE_SETS = [dict(plan="A", codes="d0")] + [dict(plan="A", sets=[f"d{j}"] if j % 2 else [f"d{j}", f"d{j + 1}"]) for j in range(1, 10)]


def _sets_step(eng, st, inp, sync):
    _enqueue_head(eng, st, inp, sync)
    return _cpu([d for per_set in eng.decode_code_sets() for d in per_set])


def test_code_set_decodes_behind_an_outstanding_handle(g1, sd):
    """Scenario 3, second variant: the same through decode_code_sets (one code set: as many counts as the plain decode; two: twice as many) while a
    decode_launch handle of the plain path is outstanding."""
    inp = _HeadInputs(g1)

    def reference():
        eng = _mk("bf16", sd)
        out = _run_sync(eng, QUEUE_SETS[:1], inp, _enqueue_head)
        for st in QUEUE_SETS[1:]:
            out.append(_sets_step(eng, st, inp, True))
            torch.cuda.synchronize()
        eng.close()
        return out
    refs = _shared("code sets", reference)
    _assert_non_vacuous(refs, _neighbours(len(refs)), "code sets behind a handle")
    assert _counts(refs[0]) != _counts(refs[8])[:2] and _counts(refs[1]) != _counts(refs[9])
    eng = _mk("bf16", sd)
    first = _run_queued(eng, QUEUE_SETS[:1], inp, _enqueue_head)[0]
    last = None
    for j, st in enumerate(QUEUE_SETS[1:], 1):
        last = _sets_step(eng, st, inp, False)
        _assert_step(last, refs[j], f"decode_code_sets {j} behind an outstanding handle")
    got = _cpu(eng.decode_fetch(first))
    _assert_step(got, refs[0], "step 0, fetched after nine code-set decodes")
    eng.close()
    fresh = _mk("bf16", sd)
    _enqueue_head(fresh, QUEUE_SETS[0], inp, True)
    _assert_same(got, _cpu(fresh.decode()), "step 0, fetched after nine code-set decodes")
    _assert_oracle(got, fresh.export_head(), inp.sizes)
    fresh.close()
    fresh = _mk("bf16", sd)
    _assert_same(last, _sets_step(fresh, QUEUE_SETS[-1], inp, True), "the last code-set decode")
    fresh.close()


# ------------------------------------------------------------------------------------------------ a status bit and its handle
QUEUE_STATUS = [dict(plan="A", heads="k32"), dict(plan="A", codes="c20", raises="candidate capacity"), dict(plan="A", heads="k16")]


def test_status_bit_travels_with_its_handle(g1, sd):
    """Scenario 4: three steps in flight on 64-slot candidate buffers (the setup of test_recovery_after_candidate_overflow): the middle one, a
    20-way head at threshold 0.011, overflows them, an error the kernel reports through the status word of that decode.  Its fetch
    raises "candidate capacity"; the steps before and after it (imported head outputs with at most 32 and 16 candidates per image and
    level) return what the synchronous engine returns."""
    cfg = _cfg(**{"MODEL.FCOS.INFERENCE_TH_TEST": 0.011})
    inp = _HeadInputs(g1)
    src = _mk("bf16", sd, cfg, cand_cap=64)
    _enqueue_head(src, dict(plan="A", codes="c20"), inp, True)
    lo, rg, ct, io = src.export_head()
    inp.heads = {"k32": (_thin(lo, 32), rg, ct, io), "k16": (_thin(lo, 16), rg, ct, io)}
    torch.cuda.synchronize()
    src.close()
    refs = _sync_reference("bf16", sd, QUEUE_STATUS, inp, _enqueue_head, cfg, cand_cap=64)
    assert refs[1] is None
    _assert_non_vacuous(refs, [(0, 2)], "status queue")
    eng = _mk("bf16", sd, cfg, cand_cap=64)
    handles = _run_queued(eng, QUEUE_STATUS, inp, _enqueue_head)
    with pytest.raises(RuntimeError, match="candidate capacity"):  # the middle handle first: the others keep their own status
        eng.decode_fetch(handles[1])
    got = {j: _cpu(eng.decode_fetch(handles[j])) for j in (0, 2)}
    for j in (0, 2):
        _assert_step(got[j], refs[j], f"status queue: step {j} of 3 in flight")
    eng.close()
    _fresh_steps("bf16", sd, QUEUE_STATUS, lambda: inp, _enqueue_head, "status queue", got, oracle=(0, 0.011, inp.heads["k32"]), cfg=cfg, cand_cap=64)


# ================================================================================================ full-path steps (scenarios 2, 5, 6)
@pytest.fixture(scope="module")
def full_sd():
    from sylph_amd import synthetic as W
    return W.synthetic_state_dict(0, depth=18)


def _full_cfg():
    """R-18: the smallest ResNet of the library.  It takes the route of the flagship's input path in bf16 (the fused stem + pool kernel
    reads the caller's images through the uploaded table), and an engine loads its weights in a quarter of R-50's time."""
    cfg = _cfg()
    cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.RESNETS.RES2_OUT_CHANNELS = 18, 64
    return cfg


@pytest.fixture(scope="module")
def streams():
    """The two extra streams of this module (scenarios 5 and 6)."""
    return [torch.cuda.Stream(), torch.cuda.Stream()]


def _ragged(sizes, seed):
    from sylph_amd import synthetic as W
    return [W.synthetic_images(1, h, w, seed=seed + i)[0] for i, (h, w) in enumerate(sizes)]


def _u8(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]


def _masters():
    """Host copies of every image set (made once); a run works on device copies of its own, since one step overwrites pixels in place."""
    def make():
        return {"X0": _ragged([(120, 150), (128, 160)], 11),             # plan (2, 128, 160)
                "X1": _ragged([(128, 140), (100, 160)], 21),             # the same plan, other sizes
                "X1b": _ragged([(128, 140), (100, 160)], 31),            # other pixels for the tensors of X1
                "Y": _ragged([(96, 128), (90, 100), (64, 128)], 41),     # plan (3, 96, 128)
                "Z0": _ragged([(128, 160), (110, 140)], 51),             # the second engine's images
                "Z1": _ragged([(80, 128), (96, 100), (70, 90)], 61),
                "U0": _u8([(60, 80), (64, 70)], 71),                     # enlarged: 3-tap resampling tables, 2 240 ints
                "U1": _u8([(192, 256), (180, 250)], 81)}                 # reduced 1.5x: 5-tap tables, 3 836 ints: more than 1.5x those of U0
    return _shared("masters", make)


U8_SIZES = {"U0": [(64, 96), (128, 160)], "U1": [(128, 150), (110, 160)]}  # both pad to 128x160: the plan of X0 and X1


class _FullInputs:
    def __init__(self):
        from sylph_amd import synthetic as W
        dev = torch.device("cuda", 0)
        self.t = {k: [im.to(dev).contiguous() for im in v] for k, v in _masters().items()}
        self.codes = {f"c{n}": {k: v.to(dev) for k, v in W.synthetic_codes(n, seed=400 + n, scale=3.0).items()} for n in (5, 7, 12, 20, 60)}
        torch.cuda.synchronize()


def _overwrite(inp, st):
    dst, src = st["overwrite"]
    for d, s in zip(inp.t[dst], inp.t[src]):
        d.copy_(s)  # on the current stream, as a serving loop refills its input buffers


def _enqueue_full(eng, st, inp, sync):
    """preprocess (or preprocess_u8) -> backbone -> head of one step, after the caller's in-place refill if the step has one."""
    if "overwrite" in st:
        _overwrite(inp, st)
    if "pre" in st:
        eng.preprocess(inp.t[st["pre"]])
    else:
        before = eng.device_bytes()  # (a host-side counter: no wait)
        eng.preprocess_u8(inp.t[st["u8"]], U8_SIZES[st["u8"]])
        if st.get("grows"):
            assert eng.device_bytes() > before, "the resize table did not outgrow the plan's previous one"
    eng.backbone()
    c = inp.codes[st["codes"]]
    if sync:
        _head(eng, c, c["cls_conv"].shape[0] > 32)
    else:
        eng.head(c["cls_conv"], c["cls_bias"])


# The issue's five paths need eight steps; all eight are in flight before the first fetch:
QUEUE_FULL = [dict(pre="X0", codes="c5"),                          # img_desc uploaded
              dict(u8="U0", codes="c20"),                          # the plan's first resize table
              dict(pre="X1", codes="c60"),                         # other ragged sizes in the same plan, behind a u8 step: uploaded
              dict(pre="X1", codes="c7"),                          # the same tensors again: no upload
              dict(pre="Y", codes="c5"),                           # a second plan in the middle
              dict(pre="X1", codes="c7", overwrite=("X1", "X1b")),  # the same tensors, refilled in place: no upload, new content
              dict(u8="U1", codes="c20", grows=True),              # the resize table outgrows the plan's previous one: reallocated
              dict(pre="X1", codes="c12")]                         # behind a u8 step with an unchanged image table: no upload


def _full_refs(full_sd):
    def reference():
        return _sync_reference("bf16", full_sd, QUEUE_FULL, _FullInputs(), _enqueue_full, _full_cfg())
    refs = _shared("full", reference)
    _assert_non_vacuous(refs, _neighbours(len(QUEUE_FULL)) + [(3, 5), (1, 6)], "full-path queue")  # (3, 5): only the pixels differ
    return refs


def test_full_path_queue_in_flight(full_sd):
    """Scenario 2: eight preprocess -> backbone -> head -> decode_launch steps in flight (QUEUE_FULL)."""
    refs = _full_refs(full_sd)
    inp = _FullInputs()
    eng = _mk("bf16", full_sd, _full_cfg())
    handles = _run_queued(eng, QUEUE_FULL, inp, _enqueue_full)
    got = {}
    for j, h in enumerate(handles):
        got[j] = _cpu(eng.decode_fetch(h))
        _assert_step(got[j], refs[j], f"full-path queue: step {j} of {len(handles)} in flight")
    eng.close()
    _fresh_steps("bf16", full_sd, QUEUE_FULL, _FullInputs, _enqueue_full, "full-path queue", got, oracle=(0, 0.05, None), cfg=_full_cfg(), share="full")


def test_full_path_queue_on_a_side_stream(full_sd, streams):
    """Scenario 5: the queue of scenario 2 issued on a non-default stream and fetched from the default stream (decode_fetch makes the current
    stream wait for the handle's), where the results are consumed."""
    refs = _full_refs(full_sd)
    inp = _FullInputs()  # (made on the default stream; synchronised)
    eng = _mk("bf16", full_sd, _full_cfg())
    torch.cuda.synchronize()
    with torch.cuda.stream(streams[0]):
        handles = _run_queued(eng, QUEUE_FULL, inp, _enqueue_full)
    assert torch.cuda.current_stream() != streams[0] and all(h[9] == streams[0] for h in handles)
    got = {}
    for j, h in enumerate(handles):
        got[j] = _cpu(eng.decode_fetch(h))  # .cpu() on the default stream
        _assert_step(got[j], refs[j], f"side-stream queue: step {j} of {len(handles)} in flight")
    torch.cuda.synchronize()
    eng.close()
    _fresh_steps("bf16", full_sd, QUEUE_FULL, _FullInputs, _enqueue_full, "side-stream queue", got, oracle=(0, 0.05, None), cfg=_full_cfg(), share="full")


# (each queue ends on its first step over again: one fresh engine serves both ends, and the last step must equal the first bit for bit)
QUEUE_TWO = {"a": [dict(pre="X0", codes="c5"), dict(pre="X1", codes="c60"), dict(pre="X0", codes="c5")],
             "b": [dict(pre="Z0", codes="c60"), dict(pre="Z1", codes="c20"), dict(pre="Z0", codes="c60")]}


def test_two_engines_on_two_streams(full_sd, streams):
    """Scenario 6: two engines, each on a stream of its own, interleaved step by step for three steps each; other images per engine, the class
    code tensors shared read-only.  Each engine's steps == that engine's synchronous reference."""
    inp = _FullInputs()
    refs = {}
    for name, steps in QUEUE_TWO.items():
        refs[name] = _sync_reference("bf16", full_sd, steps, inp, _enqueue_full, _full_cfg())
        _assert_non_vacuous(refs[name], _neighbours(len(steps)), f"engine {name}")
    for j in range(3):
        assert _differ(refs["a"][j], refs["b"][j]), f"the two engines' steps {j} have the same reference"
    engs = {name: _mk("bf16", full_sd, _full_cfg()) for name in QUEUE_TWO}
    torch.cuda.synchronize()
    handles = {name: [] for name in QUEUE_TWO}
    for j in range(3):
        for name, s in zip(QUEUE_TWO, streams):
            with torch.cuda.stream(s):
                handles[name] += _run_queued(engs[name], QUEUE_TWO[name][j:j + 1], inp, _enqueue_full)
    got = {name: {} for name in QUEUE_TWO}
    for j in range(3):
        with torch.cuda.stream(streams[0]):  # engine a from its own stream, engine b from the default stream
            got["a"][j] = _cpu(engs["a"].decode_fetch(handles["a"][j]))
        got["b"][j] = _cpu(engs["b"].decode_fetch(handles["b"][j]))
        for name in QUEUE_TWO:
            _assert_step(got[name][j], refs[name][j], f"engine {name} of two: step {j} of 3 in flight")
    torch.cuda.synchronize()
    for eng in engs.values():
        eng.close()
    for name, steps in QUEUE_TWO.items():
        _fresh_steps("bf16", full_sd, steps, lambda: inp, _enqueue_full, f"engine {name} of two", got[name],
                     oracle=(0, 0.05, None) if name == "a" else None, cfg=_full_cfg(), share="full")
