"""The forward's workspace contract on the GPU: besides the statistics pool, which the forward clears, no
byte of the workspace is assumed on entry, every buffer is written before it is read, and no kernel writes outside the
buffer it was given.

`athd_forward`, `athd_forward_prompts` and `athd_encode` run on a workspace [band | need | band] whose bytes are
prefilled: zeros (the reference run), 0xFF (NaN as f32, bf16 and f64), 0x7F (3.39e38 as f32 and bf16) or the bytes a
forward of a larger shape on another input left there, which is what AudioTextHTDemucs._workspace reuse produces.  The
outputs must not depend on the fill.  With a 64 KiB gap after every arena buffer (Arena::gap, set through
ktest.set_arena_gap) every gap must still hold its fill after the forward, and the outputs must equal the packed
layout's.  The layout itself is checked on the CPU in tests/test_workspace_refs.py.

Comparison rule: bf16 bit-identical (the claim of test_bf16_forward_reproducible: a workspace fill changes no input of
the computation); f32 within atol 1e-5, rtol 1e-4 (test_serial_matches_two_streams: same computation, other
scheduling).  The counts of differing outputs, and those of a second zero-filled run, go to
$ATHD_OUT/workspace_report.json.
"""
import ctypes

import numpy as np
import pytest
import torch

import clap_text_refs as R
import ktest as kt

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
EWORKSPACE = -5
BAND = 1 << 20                       # bytes on either side of the workspace
OUT_BAND = BAND // 4                 # floats on either side of an output
SENTINEL = -12345.5
GAP = 64 * 1024
FILL_BYTE = {"zero": 0x00, "ff": 0xFF, "7f": 0x7F}
# name: (entry, B, T, P, decode_items, seed0)
CASES = {"short": ("forward", 2, 4096, 1, kt.DEFAULT_DECODE_ITEMS, 311),
         "ragged": ("prompts", 2, 5000, 2, kt.DEFAULT_DECODE_ITEMS, 322),
         "chunks": ("prompts", 3, 1500, 2, 2, 333),
         "encode": ("encode", 2, 5000, 1, kt.DEFAULT_DECODE_ITEMS, 344)}
STALE = ("prompts", 3, 9999, 2, kt.DEFAULT_DECODE_ITEMS, 955)      # the larger shape, another input
REPORT = kt.WORKSPACE_REPORT


@pytest.fixture(autouse=True)
def _no_env_override(monkeypatch):
    monkeypatch.delenv("ATHD_DECODE_ITEMS", raising=False)      # make_dims lets it override decode_items


@pytest.fixture(scope="module")
def ctxs(state_dict):
    from athd import native
    out = {}
    for dt in DTYPES:
        c = native.Context(0, native.BF16 if dt == "bf16" else native.F32)
        for k in native.required_keys():
            c.set_weight(k, state_dict[k])
        c.finalize()
        out[dt] = c
    yield out
    for c in out.values():
        c.close()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Banded:
    """float32 [band | n | band] on the device: the sentinel in the bands, NaN inside"""

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.n = int(np.prod(self.shape))
        self.t = torch.full((self.n + 2 * OUT_BAND,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t[OUT_BAND:OUT_BAND + self.n] = float("nan")
        self.ptr = self.t.data_ptr() + 4 * OUT_BAND

    def inner(self):
        return self.t[OUT_BAND:OUT_BAND + self.n].view(self.shape)

    def bands_intact(self):
        return bool((self.t[:OUT_BAND] == SENTINEL).all() and (self.t[OUT_BAND + self.n:] == SENTINEL).all())

    def untouched(self):
        return self.bands_intact() and bool(torch.isnan(self.inner()).all())


_WAV = {}


def _inputs(case_t, text_table):
    from athd.synth import synthetic_batch
    entry, B, T, P, _, seed0 = case_t
    if (B, T, seed0) not in _WAV:
        _WAV[B, T, seed0] = torch.as_tensor(synthetic_batch(B, T, seed0=seed0)).cuda().contiguous()
    wav = _WAV[B, T, seed0]
    if entry == "forward":          # a different prompt per item
        text = torch.as_tensor(np.stack([text_table[(i + 1) % 4] for i in range(B)])).cuda().contiguous()
    else:
        text = torch.as_tensor(np.ascontiguousarray(text_table[:P])).cuda().contiguous()
    return wav, text


def _feature_outputs(B, T):
    """every tensor of athd_features, banded (x_enc, xt_enc, skip_f[0..3], skip_t[0..3], z, meant, stdt), and the struct
    that points at them"""
    from athd import native
    from athd.model import FREQ_ROWS, SKIP_CH, time_lengths
    Ts, L = -(-T // 1024), time_lengths(T)
    outs = ([Banded((B, 384, 8, Ts)), Banded((B, 384, L[4]))] + [Banded((B, SKIP_CH[i], FREQ_ROWS[i], Ts)) for i in range(4)]
            + [Banded((B, SKIP_CH[i], L[i + 1])) for i in range(4)] + [Banded((B, 2, 2048, Ts, 2)), Banded((B, 1, 1)),
                                                                         Banded((B, 1, 1))])
    f = native.Features()
    f.x_enc, f.xt_enc, f.z, f.meant, f.stdt = outs[0].ptr, outs[1].ptr, outs[10].ptr, outs[11].ptr, outs[12].ptr
    for i in range(4):
        f.skip_f[i], f.skip_t[i] = outs[2 + i].ptr, outs[6 + i].ptr
    return outs, f


def _need(ctx, case_t):
    entry, B, T, P = case_t[:4]
    return ctx.encode_workspace_bytes(B, T) if entry == "encode" else ctx.workspace_bytes(B, T, P)


def _call(ctx, case_t, wav, text, ws_ptr, ws_bytes):
    """one call of the case's entry into fresh banded outputs -> (rc, outputs)"""
    from athd import native
    entry, B, T, P = case_t[:4]
    if entry == "encode":
        outs, f = _feature_outputs(B, T)
        rc = native.lib.athd_encode(ctx.h, wav.data_ptr(), B, T, ctypes.byref(f), ws_ptr, ws_bytes, _stream())
    elif entry == "forward":
        outs = [Banded((B, 2, T))]
        rc = native.lib.athd_forward(ctx.h, wav.data_ptr(), B, T, text.data_ptr(), outs[0].ptr, ws_ptr, ws_bytes, _stream())
    else:
        outs = [Banded((B, P, 2, T))]
        rc = native.lib.athd_forward_prompts(ctx.h, wav.data_ptr(), B, T, text.data_ptr(), P, outs[0].ptr, ws_ptr,
                                             ws_bytes, _stream())
    kt.sync()
    return rc, outs


class Run:
    pass


def run(ctxs, text_table, case, dt, fill, gap):
    """The case's entry on a prefilled [band | need | band] workspace with ws_bytes == need exactly.  Checks the return
    code, that every output element was written and is finite, and every band.  -> Run: outs (the inner tensors), ws
    (the inner workspace bytes), layout, need"""
    ctx, case_t = ctxs[dt], CASES[case]
    entry, B, T, P, items, _ = case_t
    assert fill != "stale" or gap == 0
    r = Run()
    try:
        ctx.set_decode_items(items)
        kt.set_arena_gap(ctx, gap)
        r.need = _need(ctx, case_t)
        r.layout, total = kt.forward_layout(dt == "bf16", B, T, P, items, gap)
        assert r.need == total, (r.need, total)
        wav, text = _inputs(case_t, text_table)
        if fill == "stale":
            ctx.set_decode_items(STALE[4])
            big = _need(ctx, STALE)
            assert big >= r.need + BAND
            buf = torch.full((BAND + big,), 0xFF, dtype=torch.uint8, device="cuda")
            wav_b, text_b = _inputs(STALE, text_table)
            rc, _ = _call(ctx, STALE, wav_b, text_b, buf.data_ptr() + BAND, big)
            assert rc == 0, native_error(ctx)
            buf[BAND + r.need:BAND + r.need + BAND] = 0xFF          # the upper band of the small run
            ctx.set_decode_items(items)
        else:
            buf = torch.full((BAND + r.need + BAND,), 0xFF, dtype=torch.uint8, device="cuda")
            buf[BAND:BAND + r.need] = FILL_BYTE[fill]
        assert (buf.data_ptr() + BAND) % 256 == 0
        rc, outs = _call(ctx, case_t, wav, text, buf.data_ptr() + BAND, r.need)
        assert rc == 0, native_error(ctx)
    finally:
        kt.set_arena_gap(ctx, 0)
        ctx.set_decode_items(kt.DEFAULT_DECODE_ITEMS)
    assert bool((buf[:BAND] == 0xFF).all()), "bytes before the workspace were written"
    assert bool((buf[BAND + r.need:BAND + r.need + BAND] == 0xFF).all()), "bytes past the workspace were written"
    for i, o in enumerate(outs):
        assert o.bands_intact(), f"output {i}: written outside"
        bad = ~torch.isfinite(o.inner())
        assert not bool(bad.any()), (f"output {i}: {int(bad.sum())} of {o.n} elements unwritten or not finite, first at "
                                     f"flat index {int(bad.flatten().nonzero()[0])}")
    r.outs = [o.inner() for o in outs]
    r.ws = buf[BAND:BAND + r.need]
    if fill in FILL_BYTE:
        assert bool((r.ws != FILL_BYTE[fill]).any()), "the forward did not run on this workspace"
    return r


def native_error(ctx):
    from athd import native
    return native.lib.athd_last_error(ctx.h).decode()


_REF = {}        # (case, dt) -> (outputs of the zero-filled gap-0 run, differing outputs of a second such run)


def reference(ctxs, text_table, case, dt):
    key = (case, dt)
    if key not in _REF:
        a = run(ctxs, text_table, case, dt, "zero", 0).outs
        b = run(ctxs, text_table, case, dt, "zero", 0).outs
        _REF[key] = (a, _differing(a, b))
    return _REF[key]


def _differing(a, b):
    return sum(int((x.view(torch.int32) != y.view(torch.int32)).sum()) for x, y in zip(a, b))


def compare(ctxs, text_table, case, dt, outs, what):
    """the comparison rule of the module docstring against the zero-filled gap-0 run; records the counts"""
    ref, zz = reference(ctxs, text_table, case, dt)
    n = _differing(ref, outs)
    kt.record(f"{what}/{case}/{dt}", report=REPORT, differing_outputs=n, zero_vs_zero_differing=zz,
              outputs=sum(o.numel() for o in outs))
    print(f"{what} {case} {dt}: {n} outputs differ from the zero-filled run; zero against zero: {zz}")
    if dt == "bf16":
        why = ("the zero-filled run differs from its own repeat too: irreproducibility, not a stale read; rerun once "
               "with ATHD_SERIAL=1" if zz else "the zero-filled run repeats bit for bit: the workspace contents reach "
               "the output")
        assert n == 0, f"{n} outputs differ ({why})"
    else:
        for i, (o, w) in enumerate(zip(outs, ref)):
            assert torch.allclose(o, w, atol=1e-5, rtol=1e-4), (i, float((o - w).abs().max()))


@pytest.mark.parametrize("fill", ["ff", "7f", "stale"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", list(CASES))
def test_output_does_not_depend_on_workspace_contents(ctxs, text_table, case, dt, fill):
    r = run(ctxs, text_table, case, dt, fill, 0)
    compare(ctxs, text_table, case, dt, r.outs, fill)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", list(CASES))
def test_writes_stay_inside_their_buffers(ctxs, text_table, case, dt):
    r = run(ctxs, text_table, case, dt, "ff", GAP)
    live = [(n, o, b) for n, o, b in r.layout if b]
    dirty = torch.stack([(r.ws[o + b:o + b + GAP] != 0xFF).any() for _, o, b in live]).cpu().numpy()
    damaged = [f"the gap after {n} (offset {o}, {b} bytes)" for (n, o, b), d in zip(live, dirty) if d]
    assert not damaged, damaged
    compare(ctxs, text_table, case, dt, r.outs, "gap")


@pytest.mark.parametrize("dt", DTYPES)
def test_exact_size_and_refusal(ctxs, text_table, dt):
    ctx = ctxs[dt]
    for case in ("short", "ragged", "encode"):
        case_t = CASES[case]
        need = _need(ctx, case_t)
        assert need == kt.forward_layout(dt == "bf16", *case_t[1:5])[1]
        wav, text = _inputs(case_t, text_table)
        buf = torch.full((BAND + need + BAND,), 0x5A, dtype=torch.uint8, device="cuda")
        rc, outs = _call(ctx, case_t, wav, text, buf.data_ptr() + BAND, need - 1)
        assert rc == EWORKSPACE, (case, rc)
        assert str(need) in native_error(ctx)
        assert bool((buf == 0x5A).all()), case
        assert all(o.untouched() for o in outs), case


@pytest.mark.parametrize("dt", DTYPES)
def test_model_reuses_its_workspace_across_shapes(state_dict, text_table, dt):
    """AudioTextHTDemucs keeps one workspace tensor: a forward of the larger shape, then the ragged case on what it
    left, against a fresh model that runs the ragged case only."""
    from athd.model import AudioTextHTDemucs
    from athd.weights import STEMS

    def model():
        m = AudioTextHTDemucs(dtype=dt, text_table={s: text_table[i] for i, s in enumerate(STEMS)})
        m.load_state_dict(state_dict)
        return m.to("cuda").eval()

    wav_b, _ = _inputs(STALE, text_table)
    wav, _ = _inputs(CASES["ragged"], text_table)
    prompts = list(STEMS[:2])
    m = model()
    big = m.forward_prompts(wav_b, prompts)
    ws = m._ws
    reused = m.forward_prompts(wav, prompts)
    assert m._ws is ws                                  # the smaller shape ran on the larger one's workspace
    fresh = model().forward_prompts(wav, prompts)
    kt.sync()
    assert bool(torch.isfinite(big).all()) and bool(torch.isfinite(reused).all())
    n = _differing([fresh], [reused])
    kt.record(f"model_reuse/{dt}", report=REPORT, differing_outputs=n, outputs=reused.numel())
    if dt == "bf16":
        assert n == 0, f"{n} outputs differ (if test_bf16_forward_reproducible fails too: rerun once with ATHD_SERIAL=1)"
    else:
        assert torch.allclose(reused, fresh, atol=1e-5, rtol=1e-4), float((reused - fresh).abs().max())


# ---- the text tower: no atomics, so bit-identical in both dtypes ----
@pytest.mark.parametrize("dt", DTYPES)
def test_text_tower_does_not_depend_on_workspace_contents(dt):
    from athd import native
    from athd.text import NativeClapText
    from athd.weights import synthetic_clap_text_state_dict
    nat = NativeClapText("cuda", dtype=dt)
    nat.load_state_dict(synthetic_clap_text_state_dict(R.SEED))
    ctx = nat._ensure_ctx()
    ids, mask = R.CASES["ragged9"]
    assert tuple(int(v) for v in np.asarray(mask).sum(axis=1)) == R.RAGGED
    ids = torch.as_tensor(np.asarray(ids)).to(torch.int32).cuda().contiguous()
    mask = torch.as_tensor(np.asarray(mask)).to(torch.int32).cuda().contiguous()
    P, L = ids.shape
    need = ctx.workspace_bytes(P, L)
    assert need > 0
    got = {}
    for fill, byte in FILL_BYTE.items():
        buf = torch.full((BAND + need + BAND,), 0xFF, dtype=torch.uint8, device="cuda")
        buf[BAND:BAND + need] = byte
        out = Banded((P, 512))
        rc = native.lib.athd_text_encode(ctx.h, ids.data_ptr(), mask.data_ptr(), P, L, 0, out.ptr, buf.data_ptr() + BAND,
                                         need, _stream())
        kt.sync()
        assert rc == 0, fill
        assert bool((buf[:BAND] == 0xFF).all()) and bool((buf[BAND + need:] == 0xFF).all()), fill
        assert out.bands_intact() and bool(torch.isfinite(out.inner()).all()), fill
        got[fill] = out.inner()
    for fill in ("ff", "7f"):
        n = _differing([got["zero"]], [got[fill]])
        kt.record(f"text_tower/{fill}/{dt}", report=REPORT, differing_outputs=n, outputs=P * 512)
        assert n == 0, (fill, n)
