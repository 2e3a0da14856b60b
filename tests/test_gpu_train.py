"""The training ends on the GPU: `athd_loss_grad_coef`, `athd_loss_grad_apply`, `athd_gather_train_segments`,
athd/loss.py `loss_with_grad`, athd/train_data.py and athd/train.py.

  1. Gradient parity against float64 autograd of the losses written out in tests/train_refs.py (not the closed form the
     kernel evaluates).  Bound, per row: max |grad - g64| <= 2^-23 max |g64|.  Derived, not measured: the kernel
     evaluates each element once in fp64 and rounds once to f32, which is within 2^-24 of the element, hence of the
     row's largest; the factor 2 is the margin for the fp64 coefficients.  Shapes: one element, tails, odd n, n = 60002
     (past the 16384-element chunk: a row spans several blocks) and (2, 88200), the reference's gradient-flow check;
     est, target and grad aligned, all one float in, est only, grad only.  Families snr, dc and clamp with no row
     within 0.01 dB of a clamp, so the float64 reference alone decides every gate; both losses; under the L1 loss row 0
     has e_i == t_i at every third element.  Rows whose float64 gradient is all zero are exactly zero.  The worst ratio
     is printed next to the fixture's a (the reference's own f32 autograd against float64).
  2. `table` of athd_loss_grad_coef has the bits of athd_loss_rows; `combined_loss(e.requires_grad_())` returns the
     bits and the dict of the call without grad.
  3. an upstream gradient of 1024, a transposed and a bfloat16 `estimated`, the refused calls.
  4. coef and grad are the same bits run to run and from a captured graph.
  5. `athd_gather_train_segments` is bit-exact against the numpy restatement and, on the recorded plans, against the
     reference's own items (tests/golden/train_ref.npz).
  6. three steps of `train_epoch` against the same loop around the float64 loss: parameters within 1e-5 relative, the
     returned dict within 1e-4 dB.
"""
import copy
import os
import random

import numpy as np
import pytest
import torch

import train_refs as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -23
SHAPES = [(1, 1), (3, 63), (5, 74), (4, 257), (5, 3002), (2, 60002), (2, 88200)]
WEIGHTS = {"combined": lambda w1, w2: (w1, w2, 0.0), "combined_l1": lambda w1, w2: (w1, 0.0, w2)}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "train_ref.npz"))


def _offset_view(x: torch.Tensor) -> torch.Tensor:
    """The same values in a device view that starts one float into a larger allocation."""
    buf = torch.empty(x.numel() + 5, dtype=torch.float32, device="cuda")
    buf[1:1 + x.numel()] = x.reshape(-1).cuda()
    v = buf[1:1 + x.numel()].view(x.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _native_grad(est, tgt, weights, upstream=None, grad=None):
    """(table, coef, grad) straight from the C ABI on device tensors; `grad` may be a caller's (misaligned) buffer."""
    from athd import native
    rows, n = est.shape
    scratch = torch.empty(native.lib.athd_loss_grad_scratch_bytes(rows, n) // 8, dtype=torch.float64, device="cuda")
    table = torch.empty((rows, 4), dtype=torch.float64, device="cuda")
    coef = torch.empty((rows, 8), dtype=torch.float64, device="cuda")
    grad = torch.empty((rows, n), dtype=torch.float32, device="cuda") if grad is None else grad
    assert native.lib.athd_loss_grad_coef(est.data_ptr(), tgt.data_ptr(), rows, n, scratch.data_ptr(),
                                          table.data_ptr(), coef.data_ptr(), _stream()) == 0
    assert native.lib.athd_loss_grad_apply(est.data_ptr(), tgt.data_ptr(), rows, n, coef.data_ptr(), *weights,
                                           None if upstream is None else upstream.data_ptr(), grad.data_ptr(),
                                           _stream()) == 0
    return table, coef, grad


def _inputs(family, rows, n, loss):
    est, tgt = R.FAMILIES[family](rows, n)
    assert R.clamp_margin(est, tgt) > 0.01
    if loss == "combined_l1" and n >= 3:
        est, tgt = R.with_ties(est, tgt)
        assert R.clamp_margin(est, tgt) > 0.01 and int((est[0] == tgt[0]).sum()) >= n // 3
    return est, tgt


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
@pytest.mark.parametrize("rows,n", SHAPES)
def test_gradient_matches_float64_autograd(rows, n, family, fx):
    from athd.loss import loss_rows
    for loss, (w1, w2) in R.LOSSES.items():
        est, tgt = _inputs(family, rows, n, loss)
        want = R.grad64(est, tgt, loss)
        ea, ta, e1, t1 = est.cuda(), tgt.cuda(), _offset_view(est), _offset_view(tgt)
        cases = {"aligned": (ea, ta, None), "all one float in": (e1, t1, _offset_view(torch.zeros(rows, n))),
                 "est one float in": (e1, ta, None), "grad one float in": (ea, ta, _offset_view(torch.zeros(rows, n)))}
        for what, (e, t, g) in cases.items():
            table, _, got = _native_grad(e, t, WEIGHTS[loss](w1, w2), grad=g)
            assert torch.equal(table, loss_rows(e, t)), (loss, what)
            got = got.cpu().numpy()
            assert np.isfinite(got).all()
            ratio = R.row_gap(got, want) / BOUND
            print(f"loss grad {loss} {family} ({rows}, {n}) {what}: worst row error {ratio:.3f} x 2^-23 of the row's "
                  f"largest |gradient| (<= 1; the reference's own f32 autograd: {float(fx['a']) / BOUND:.3f})")
            assert ratio <= 1.0, (loss, family, rows, n, what, ratio)


def test_l1_gradient_is_zero_where_estimate_equals_target():
    est, tgt = _inputs("snr", 3, 63, "combined_l1")
    tgt[0] = est[0]                      # the whole row: raw SDR beyond +30 dB, so only the L1 term could contribute
    _, _, got = _native_grad(est.cuda(), tgt.cuda(), (1.0, 0.0, 0.05))
    assert not got[0].any() and got[1:].abs().min() > 0
    assert not np.any(R.grad64(est, tgt, "combined_l1")[0])


@pytest.mark.parametrize("loss", sorted(R.LOSSES))
def test_differentiable_value_has_the_same_bits(loss):
    import athd.loss as L
    fn = L.combined_loss if loss == "combined" else L.combined_L1_sdr_loss
    for family in sorted(R.FAMILIES):
        est, tgt = R.FAMILIES[family](5, 3002)
        e, t = est.reshape(5, 2, 1501).cuda(), tgt.reshape(5, 2, 1501).cuda()
        plain, metrics = fn(e, t)
        assert plain.grad_fn is None and not plain.requires_grad
        with torch.no_grad():
            off, _ = fn(e.clone().requires_grad_(True), t)
        assert off.grad_fn is None
        total, metrics_grad = fn(e.clone().requires_grad_(True), t)
        assert total.requires_grad and total.dtype == torch.float32 and total.dim() == 0
        assert torch.equal(total.detach().view(torch.int32), plain.view(torch.int32)), (loss, family)
        assert metrics_grad == metrics and list(metrics_grad) == list(metrics)


def test_backward_reaches_the_estimate_and_scales_with_upstream():
    from athd.loss import combined_loss
    est, tgt = R.FAMILIES["snr"](4, 257)
    want = R.grad64(est, tgt, "combined")
    e = est.cuda().requires_grad_(True)
    combined_loss(e, tgt.cuda())[0].backward()
    assert R.row_gap(e.grad.cpu().numpy(), want) <= BOUND
    e2 = est.cuda().requires_grad_(True)
    (combined_loss(e2, tgt.cuda())[0] * 1024).backward()
    gap = R.row_gap(e2.grad.cpu().numpy(), 1024 * want)
    print(f"upstream 1024: worst row error {gap / BOUND:.3f} x 2^-23")
    assert gap <= BOUND
    # a transposed view: the gradient reaches the (n, rows) leaf and is the contiguous result permuted
    base = est.t().contiguous().cuda().requires_grad_(True)
    assert not base.t().is_contiguous()
    combined_loss(base.t(), tgt.cuda())[0].backward()
    assert torch.equal(base.grad, e.grad.t())
    # a bfloat16 estimate: the cast is a torch op outside the Function, the gradient comes back in bfloat16
    h = est.cuda().bfloat16().requires_grad_(True)
    combined_loss(h, tgt.cuda())[0].backward()
    f = h.detach().float().requires_grad_(True)
    combined_loss(f, tgt.cuda())[0].backward()
    assert h.grad.dtype == torch.bfloat16 and torch.equal(h.grad, f.grad.bfloat16())


def test_refused_calls_write_nothing():
    from athd import native
    from athd.loss import combined_loss, loss_with_grad
    x = torch.zeros(16, device="cuda")
    with pytest.raises(ValueError, match="target must not require grad"):
        loss_with_grad(x.reshape(2, 8).requires_grad_(True), x.reshape(2, 8).clone().requires_grad_(True), 0.9, 0.1, 0.0)
    with pytest.raises(ValueError, match="target must not require grad"):
        combined_loss(x.reshape(2, 8).requires_grad_(True), x.reshape(2, 8).clone().requires_grad_(True))
    s = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    table = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    coef = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    grad = torch.full((16,), 7.0, device="cuda")
    p = lambda v: None if v is None else v.data_ptr()
    for rows, n, e, c in ((0, 4, x, coef), (1, 0, x, coef), (1, 1 << 31, x, coef), ((1 << 20) + 1, 1, x, coef),
                          (1, 4, None, coef), (1, 4, x, None)):
        assert native.lib.athd_loss_grad_coef(p(e), p(x), rows, n, p(s), p(table), p(c), None) == -1
        assert native.lib.athd_loss_grad_apply(p(e), p(x), rows, n, p(c), 0.9, 0.1, 0.0, None, p(grad), None) == -1
    assert native.lib.athd_loss_grad_coef(p(x), p(x), 1, 4, None, p(table), p(coef), None) == -1
    assert native.lib.athd_loss_grad_apply(p(x), p(x), 1, 4, p(coef), 0.9, 0.1, 0.0, None, None, None) == -1
    torch.cuda.synchronize()
    for buf in (s, table, coef, grad):
        assert bool((buf == 7.0).all())


@pytest.mark.parametrize("rows,n", [(5, 3002), (2, 60002)])
def test_deterministic_and_capturable(rows, n):
    est, tgt = R.FAMILIES["dc"](rows, n, seed=4)
    est, tgt = _offset_view(est), _offset_view(tgt)
    up = torch.tensor(3.0, device="cuda")
    weights = (0.9, 0.1, 0.05)
    _, coef_a, grad_a = _native_grad(est, tgt, weights, up)
    _, coef_b, grad_b = _native_grad(est, tgt, weights, up)
    assert torch.equal(coef_a, coef_b) and torch.equal(grad_a, grad_b) and bool(grad_a.any())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, coef_c, grad_c = _native_grad(est, tgt, weights, up)
    coef_c.zero_()
    grad_c.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(coef_a, coef_c) and torch.equal(grad_a, grad_c)


# ------------------------------------------------------------------------------------------- train segments
STARTS = [0, 1, 743, 744, 745, 999, 1000]
GAINS = [1.0, 0.7, 1.3, random.Random(12).uniform(0.7, 1.3)]


def _segment_case(stems_np, stems_dev, starts, seg):
    from athd.train_data import gather_train_segments
    rows = [(s, st, g, sw) for s in range(stems_np.shape[0]) for st in starts for g in GAINS for sw in (False, True)]
    got = gather_train_segments(stems_dev, *[[r[k] for r in rows] for k in range(4)], seg).cpu().numpy()
    assert got.shape == (len(rows), 2, seg)
    for k, (s, st, g, sw) in enumerate(rows):
        assert np.array_equal(got[k], R.train_segment_ref(stems_np, s, st, g, sw, seg)), (s, st, g, sw)
    return got, rows


def test_train_segments_bit_exact():
    from athd.validate import gather_segments
    rng = np.random.default_rng(5)
    stems = rng.standard_normal((3, 1000, 2)).astype(np.float32)
    aligned = torch.from_numpy(stems).cuda()
    assert aligned.data_ptr() % 8 == 0
    got, rows = _segment_case(stems, aligned, STARTS, 256)
    at = rows.index((1, 745, 1.0, False))
    assert np.all(got[at][:, 255:] == 0) and np.all(got[at][:, :255] != 0)        # 255 real frames, then zeros
    assert not got[rows.index((2, 1000, 1.3, True))].any()                        # a start at the end: all padding
    _segment_case(stems, _offset_view(torch.from_numpy(stems)), STARTS, 256)      # base 4 (mod 8): the 4-byte loads
    short = rng.standard_normal((3, 100, 2)).astype(np.float32)                   # a track shorter than one segment
    _segment_case(short, torch.from_numpy(short).cuda(), [0, 1, 99, 100], 256)
    _segment_case(short, _offset_view(torch.from_numpy(short)), [0, 1, 99, 100], 256)
    # gain 1, no swap, start on the grid: athd_gather_segments
    from athd.train_data import gather_train_segments
    src, seg = [0, 1, 2, 2], [0, 2, 3, 1]
    assert torch.equal(gather_train_segments(aligned, src, [s * 256 for s in seg], [1.0] * 4, [False] * 4, 256),
                       gather_segments(aligned, src, seg, 256))


def test_train_segments_out_of_range_rows_are_zero():
    from athd import native
    stems = torch.ones((2, 10, 2), device="cuda")
    src = torch.tensor([0, 2, -1, 1, 1, 1, 0], dtype=torch.int32, device="cuda")
    start = torch.tensor([3, 0, 0, -1, 11, 2 ** 63 - 1, 10], dtype=torch.int64, device="cuda")
    gain = torch.full((7,), 2.0, dtype=torch.float64, device="cuda")
    swap = torch.zeros(7, dtype=torch.uint8, device="cuda")
    out = torch.full((7, 2, 4), 7.0, device="cuda")
    call = lambda stems_p, rows: native.lib.athd_gather_train_segments(
        stems_p, 2, 10, src.data_ptr(), start.data_ptr(), gain.data_ptr(), swap.data_ptr(), rows, 4, out.data_ptr(),
        _stream())
    assert call(None, 7) == -1 and call(stems.data_ptr(), 0) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(stems.data_ptr(), 7) == 0
    assert torch.equal(out[0], torch.full((2, 4), 2.0, device="cuda")) and float(out[1:].abs().max()) == 0.0


@pytest.fixture(scope="module")
def dataset(fx, tmp_path_factory):
    from athd.musdb import MusDBTracks
    from athd.train_data import TrainSegmentDataset
    root = tmp_path_factory.mktemp("train_tracks")
    for i, length in enumerate(fx["track_lengths"]):
        np.save(root / f"track{i}.stem.npy", R.train_track(int(length)))
    return TrainSegmentDataset(MusDBTracks(root), int(fx["segment_samples"]))


def test_gather_reproduces_reference_items(fx, dataset):
    from athd.musdb import STEM_NAMES
    from athd.train_data import Plan
    n = len(fx["item_prompt"])
    plans = [Plan(int(fx["item_file"][i]), STEM_NAMES.index(str(fx["item_stem"][i])), int(fx["item_segment"][i]),
                  int(fx["plan_start"][i]), float(fx["plan_gain"][i]), bool(fx["plan_swap"][i]),
                  str(fx["item_prompt"][i])) for i in range(n)]
    for fi in sorted({p.file_idx for p in plans}):
        pos = [i for i, p in enumerate(plans) if p.file_idx == fi]
        mixtures, targets = dataset.gather(fi, [plans[i] for i in pos], "cuda")
        assert np.array_equal(mixtures.cpu().numpy(), fx["item_mixture"][pos])
        assert np.array_equal(targets.cpu().numpy(), fx["item_target"][pos])
    with pytest.raises(ValueError, match="must belong to track"):
        dataset.gather(0, plans, "cuda")
    # the collated batch: the same draws in loader order, items of both tracks in one batch
    random.seed(R.ITEMS_SEED)
    batch = dataset.batch(range(n), "cuda")
    assert random.random() == float(fx["random_after"])
    assert np.array_equal(batch["mixture"].cpu().numpy(), fx["item_mixture"])
    assert np.array_equal(batch["target"].cpu().numpy(), fx["item_target"])
    assert batch["prompt"] == [str(p) for p in fx["item_prompt"]]
    assert batch["stem_name"] == [str(s) for s in fx["item_stem"]]


# ------------------------------------------------------------------------------------------------ end to end
class PointwiseNet(torch.nn.Conv1d):
    """`torch.nn.Conv1d(2, 2, 1)` behind the model's call signature."""

    def __init__(self):
        super().__init__(2, 2, 1)
        g = torch.Generator().manual_seed(31)
        with torch.no_grad():
            self.weight.copy_(torch.eye(2)[:, :, None] + 0.1 * torch.randn(2, 2, 1, generator=g))
            self.bias.copy_(0.01 * torch.randn(2, generator=g))

    def forward(self, mixture, prompts):
        assert len(prompts) == mixture.shape[0]
        return super().forward(mixture)


def _batches():
    out = []
    for k in range(3):
        est, tgt = R.FAMILIES["snr"](4, 6004, seed=40 + k)
        out.append({"mixture": est.reshape(4, 2, 3002).cuda(), "target": tgt.reshape(4, 2, 3002).cuda(),
                    "prompt": ["drums", "bass", "other instruments", "vocals"]})
    return out


def _run_pair(kind, w1, w2, **kw):
    from athd.train import train_epoch
    batches = _batches()
    mine, ref = PointwiseNet().cuda(), PointwiseNet().cuda()
    with torch.no_grad():
        for b in batches:
            assert R.clamp_margin(ref(b["mixture"], b["prompt"]).cpu(), b["target"].cpu()) > 0.5
    opt_mine = torch.optim.AdamW(mine.parameters(), lr=1e-3)
    opt_ref = torch.optim.AdamW(ref.parameters(), lr=1e-3)
    got = train_epoch(mine, batches, opt_mine, None, "cuda", False, grad_clip=1.0, epoch=0, log_every=0, **kw)
    want = R.train_epoch_ref(ref, batches, opt_ref, kind, w1, w2, 1.0)
    assert list(got) == ["loss", "sdr", "sisdr"]
    worst = max(abs(got[k] - want[k]) for k in want)
    start = PointwiseNet()
    rel = 0.0
    for (name, a), b, p0 in zip(mine.named_parameters(), ref.parameters(), start.parameters()):
        assert float((a.detach().cpu() - p0.detach()).abs().max()) > 1e-4, name          # three AdamW steps of 1e-3 moved it
        rel = max(rel, float(((a - b).abs() / b.abs()).max().detach()))
    print(f"train_epoch {kind}: parameters within {rel:.3e} relative (<= 1e-5), dict within {worst:.3e} dB (<= 1e-4)")
    assert rel <= 1e-5 and worst <= 1e-4, (kind, rel, got, want)


def test_train_epoch_three_steps_match_float64_loss():
    _run_pair("combined", 0.9, 0.1, use_L1_cmb_loss=False, l1_sdr_weight=None, l1_weight=None, sdr_weight=0.9,
              sisdr_weight=0.1)


def test_train_epoch_l1_variant_and_errors():
    from athd.train import train_epoch
    _run_pair("combined_l1", 1.0, 0.05, use_L1_cmb_loss=True, l1_sdr_weight=1.0, l1_weight=0.05, sdr_weight=0.9,
              sisdr_weight=0.1)
    net = PointwiseNet().cuda()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="l1_weight must be provided"):
        train_epoch(net, _batches(), opt, None, "cuda", False, True, 1.0, None, 1.0, 0.9, 0.1, 0, 0)
    with pytest.raises(ValueError, match="wandb"):
        train_epoch(net, _batches(), opt, None, "cuda", False, False, None, None, 1.0, 0.9, 0.1, 0, 0, use_wandb=True)


def test_train_epoch_amp_branch_steps():
    from athd.train import train_epoch
    net = PointwiseNet().cuda()
    before = copy.deepcopy(net.state_dict())
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    # a dB loss has parameter gradients of order 10: the default scale of 65536 overflows their fp16 form and the
    # scaler would skip (and halve) through all three steps, as it would around the reference's loss
    scaler = torch.amp.GradScaler("cuda", init_scale=16.0)
    got = train_epoch(net, _batches(), opt, scaler, "cuda", True, False, None, None, 1.0, 0.9, 0.1, 0, 0)
    assert all(np.isfinite(v) for v in got.values())
    for k, v in net.state_dict().items():
        assert torch.isfinite(v).all() and float((v - before[k]).abs().max()) > 1e-4, k
    assert scaler.get_scale() == 16.0                    # no step was skipped
