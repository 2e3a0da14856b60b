"""The forward's workspace layout (csrc/forward_plan.cpp plan(), through ktest.forward_layout), on the CPU: offsets and
order, the total against the values of the commit before Arena::gap existed, what a gap changes and what it must not,
the null slots, and the decoder buffers' sizes against a second derivation from what the decoder levels write
(csrc/forward_dec.cpp), which does not use plan()'s max expressions.  The GPU half is tests/test_gpu_workspace.py.
"""
import pytest

import ktest as kt

DTYPES = ["f32", "bf16"]
GAP = 64 * 1024
# name: (B, T, P, decode_items); the first four are the cases of tests/test_gpu_workspace.py, then its stale shape and
# the bench shape
SHAPES = {"short": (2, 4096, 1, 64), "ragged": (2, 5000, 2, 64), "chunks": (3, 1500, 2, 2), "encode": (2, 5000, 1, 64),
          "stale": (3, 9999, 2, 64), "bench": (64, 264600, 4, 256)}
# athd_workspace_bytes of the commit before Arena::gap (its plan() run on a null arena, decode_items as above).  The
# bf16 values hold for a device of 256 CUs and for no device (fdec1f.hip sizes its partial slots by the CU count).
PARENT_BYTES = {
    ("short", "f32"): 10273280, ("ragged", "f32"): 16525056, ("chunks", "f32"): 6354432,
    ("encode", "f32"): 12713472, ("stale", "f32"): 48983552, ("bench", "f32"): 59406454528,
    ("short", "bf16"): 216738816, ("ragged", "bf16"): 221927424, ("chunks", "bf16"): 213963520,
    ("encode", "bf16"): 218371840, ("stale", "bf16"): 245239808, ("bench", "bf16"): 49480596736,
}
BF16_ONLY = {"hbuf_b_t", "hbuf_b", "x_enc_b", "xt_enc_b", "gram", "gramq", "skw0", "skw1"}


@pytest.fixture(autouse=True)
def _no_env_override(monkeypatch):
    monkeypatch.delenv("ATHD_DECODE_ITEMS", raising=False)      # make_dims lets it override decode_items


def _layout(shape, dt, gap=0):
    B, T, P, items = SHAPES[shape]
    return kt.forward_layout(dt == "bf16", B, T, P, items, gap)


def _live_checked(slots):
    """the non-null slots, after checking: 256-aligned, strictly increasing, pairwise disjoint"""
    live = [(n, o, b) for n, o, b in slots if b]
    for n, o, b in live:
        assert o % 256 == 0 and b % 256 == 0 and b > 0, (n, o, b)
    for (n0, o0, b0), (n1, o1, _) in zip(live, live[1:]):
        assert o0 < o1 and o0 + b0 <= o1, (n0, o0, b0, n1, o1)     # sorted, so disjoint from every later one too
    return live


def _chunks(B, P, items):
    Bc = max(1, min(B, items // P))
    return Bc, -(-B // Bc)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_offsets_order_and_total(shape, dt):
    slots, total = _layout(shape, dt)
    assert [n for n, _, _ in slots] == kt.LAYOUT_NAMES
    live = _live_checked(slots)
    end = 0
    for n, o, b in live:
        assert o == end, (n, o, end)                               # gap 0: packed from offset 0
        end = o + b
    assert end == total
    assert total == PARENT_BYTES[shape, dt]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gap_shifts_offsets_only(shape, dt):
    s0, t0 = _layout(shape, dt)
    sg, tg = _layout(shape, dt, GAP)
    live0, liveg = _live_checked(s0), _live_checked(sg)
    assert [n for n, _, _ in live0] == [n for n, _, _ in liveg]
    for i, ((n, o0, b0), (_, og, bg)) in enumerate(zip(live0, liveg)):
        assert og == o0 + i * GAP and bg == b0, (n, i, o0, og, b0, bg)
    assert tg == t0 + len(live0) * GAP
    assert {n for n, _, b in s0 if not b} == {n for n, _, b in sg if not b}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_null_slots(shape, dt):
    B, T, P, items = SHAPES[shape]
    null = {n for n, _, b in _layout(shape, dt)[0] if not b}
    want = set() if dt == "bf16" else set(BF16_ONLY)
    if _chunks(B, P, items)[1] == 1:
        want.add("FO2")
    assert null == want


def test_chunked_case_has_three_chunks():
    B, T, P, items = SHAPES["chunks"]
    assert _chunks(B, P, items) == (1, 3)


# ---- the decoder buffers, from what the decoder levels write (forward_dec.cpp) ----
def decoder_needs(bf16, Bc, P, T, chunks):
    """bytes a consumer needs of each decoder buffer, for one decode chunk of Bc segments x P prompts.  e: bytes of an
    activation element (the ConvT / merge / tap-product buffers hold bf16 in bf16 mode); the two output stages and the
    iSTFT's partial sums are fp32 in both modes."""
    e = 2 if bf16 else 4
    NI = Bc * P
    Ts = -(-T // 1024)
    L = [T]
    for _ in range(4):
        L.append(-(-L[-1] // 4))
    need = {}
    # frequency branch.  level 0: ConvT of 8 rows -> 32 rows x Ts frames x 192 channels, all rows stored; GroupNorm +
    # GELU in place (f32) or into S (bf16).  level 1 reads those 32 rows (and the skip's 8 rows) through per-tap
    # products of 8 taps x 96 channels and writes Ts rows x Ts frames x 96.  level 2: ConvT of Ts rows -> 4 Ts, of
    # which rows 4u+1, 4u+2 are stored: 2 Ts rows x Ts frames x 48.  The folded last level writes [NI][Ts][Ts][2] fp32.
    convt0 = NI * 32 * Ts * 192 * e
    need["G"] = max(convt0, NI * 2 * Ts * Ts * 48 * e)
    need["S"] = convt0 if bf16 else 0
    need["Z"] = NI * 32 * Ts * (8 * 96) * e
    need["Zs"] = Bc * 8 * Ts * (8 * 96) * e
    need["D"] = NI * Ts * Ts * 96 * e
    need["FO"] = NI * Ts * Ts * 2 * 4
    if chunks > 1:
        need["FO2"] = need["FO"]
    # time branch.  level i: ConvT of Lin rows -> 4 Lin rows x cout into Gt, merged (resized) to L[3 - i] rows x cout
    # into Dt.  The last level writes xt2 [NI][T][2] fp32: into Dt when it is fused with level 2's merge (only when
    # 4 L1 == T), else into Gt.
    gt, dtb, Lin = 0, 0, L[4]
    for i, cout in enumerate((192, 96, 48)):
        gt = max(gt, NI * 4 * Lin * cout * e)
        Lin = L[3 - i]
        dtb = max(dtb, NI * Lin * cout * e)
    xt2 = NI * T * 2 * 4
    need["Gt"] = max(gt, xt2)
    need["Dt"] = max(dtb, xt2) if 4 * L[1] == T else dtb
    # iSTFT: per item and workgroup, {head, tail} x 3 blocks x 4 offsets x 256 threads x 2 channels of fp32
    # (spectral.hip ola_part)
    need["ola_part"] = NI * kt.lib.kt_istft_nwg(Ts) * 2 * 3 * 4 * 256 * 2 * 4
    return need


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,P,items", [(2, 2, 64), (3, 2, 2), (2, 1, 64)])
@pytest.mark.parametrize("T", [1, 1023, 1024, 1025, 1500, 4096, 5000, 9999, 33297])
def test_decoder_buffers_hold_what_the_levels_write(T, B, P, items, dt):
    Bc, chunks = _chunks(B, P, items)
    have = {n: b for n, _, b in kt.forward_layout(dt == "bf16", B, T, P, items)[0]}
    need = decoder_needs(dt == "bf16", Bc, P, T, chunks)
    assert set(need) >= {"G", "D", "Gt", "Dt", "S", "Z", "Zs", "FO", "ola_part"}
    short = {n: (have[n], v) for n, v in need.items() if have[n] < v}
    assert not short, short
