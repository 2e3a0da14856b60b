"""The references of head training's update step are sound, and the bound the GPU tests use is reachable (no GPU).

  1. `ref64` is torch's step: against `clip_grad_norm_` + `torch.optim.AdamW` in float64 it agrees to 1e-13.
  2. A float32 evaluation stays within ALLOW x the gap of torch's own float32 step to `ref64`: both the kernel's form
     (float32 storage, float64 arithmetic, one rounding per stored value) and plain float32 arithmetic.
  3. Every planted defect exceeds that allowance in the regime named for it (head_step_refs.MUTATIONS).
  4. `HeadAdamW`'s `state_dict()` has `torch.optim.AdamW`'s layout key for key, and each loads the other's; the
     constructor refuses what `athd_head_step` does not cover.  (The kernel needs a GPU; the host-side state handling is
     checked here on a subclass that lifts the device check alone.)
"""
import numpy as np
import pytest
import torch

import head_step_refs as R

KS = [1, 3]


@pytest.mark.parametrize("regime", list(R.REGIMES))
@pytest.mark.parametrize("K", KS)
def test_ref64_is_torch_float64(regime, K):
    c = R.case(regime)
    want = R.ref64(c, K)
    got, _, _ = R.torch_step(c, K, torch.float64)
    g = R.gaps(got, want, c["p0"])
    assert max(g.values()) <= 1e-13, g
    if regime == "inactive":
        assert all(x == 1.0 for x in want["coef"])
    if regime == "active":
        assert all(x < 0.01 for x in want["coef"])


@pytest.mark.parametrize("regime", list(R.REGIMES))
@pytest.mark.parametrize("K", KS)
def test_float32_reaches_the_bound_and_defects_do_not(regime, K):
    c = R.case(regime)
    want = R.ref64(c, K)
    a = R.gaps(R.torch_step(c, K, torch.float32)[0], want, c["p0"])
    print(regime, K, "torch f32 gap:", a)
    assert all(0.0 < a[k] < 1e-4 for k in a), a
    for name, kw in (("kernel form", dict(store=np.float32)), ("float32", dict(store=np.float32, arith=np.float32))):
        g = R.gaps(R.ref64(c, K, **kw), want, c["p0"])
        print(" ", name, {k: g[k] / a[k] for k in g})
        for k in g:
            assert g[k] <= R.ALLOW * a[k], (name, k, g[k], a[k])
    for mut, where in R.MUTATIONS.items():
        if where != regime:
            continue
        g = R.gaps(R.ref64(c, K, mut=mut), want, c["p0"])
        print("  defect", mut, g["disp"], "allowed", R.ALLOW * a["disp"])
        assert g["disp"] > 100 * R.ALLOW * a["disp"], (mut, g, a)


def test_grad_scale_is_exact_for_a_power_of_two():
    c = R.case("inactive")
    scaled = {"p0": c["p0"], "grads": [[8.0 * g for g in gs] for gs in c["grads"]]}
    a, b = R.ref64(c, 3, store=np.float32), R.ref64(scaled, 3, store=np.float32, grad_scale=8.0)
    for k in ("p", "m", "v"):
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k


class _HostAdamW:
    """`HeadAdamW` with the device check lifted: the state handling on CPU tensors (no step)"""

    def __new__(cls, *a, **kw):
        from athd.optim import HeadAdamW

        class Host(HeadAdamW):
            _check_params = staticmethod(lambda params: None)

        return Host(*a, **kw)


def _params():
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((3, 5), (7,), (2, 2, 2))]


def test_state_dict_layout_is_adamw():
    params = _params()
    ref = torch.optim.AdamW(params, lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.1)
    for k in range(2):
        for p in params:
            p.grad = torch.full_like(p, 0.1 * (k + 1))
        ref.step()
    want = ref.state_dict()
    host = _HostAdamW(params, lr=1e-3)
    host.load_state_dict(want)                                            # AdamW -> HeadAdamW
    assert host.step_count() == 2
    for p in params:
        assert set(host.state[p]) == {"exp_avg", "exp_avg_sq"}
        assert host.state[p]["exp_avg"].data_ptr() % 16 == 0 and host.state[p]["exp_avg_sq"].data_ptr() % 16 == 0
    got = host.state_dict()
    assert list(got) == list(want)
    assert [set(g) for g in got["param_groups"]] == [set(g) for g in want["param_groups"]]
    assert got["param_groups"][0]["lr"] == 2e-3 and got["param_groups"][0]["betas"] == (0.8, 0.99)
    assert set(got["state"]) == set(want["state"])
    for i, w in want["state"].items():
        assert list(got["state"][i]) == list(w)                           # step, exp_avg, exp_avg_sq, in this order
        for k in w:
            assert got["state"][i][k].dtype == w[k].dtype and got["state"][i][k].device == w[k].device, k
            assert torch.equal(got["state"][i][k], w[k]), k
    # a fresh one has AdamW's group keys too, and an empty state
    fresh = _HostAdamW(params, lr=1e-3).state_dict()
    plain = torch.optim.AdamW(params, lr=1e-3).state_dict()
    assert fresh["state"] == {} and set(fresh["param_groups"][0]) == set(plain["param_groups"][0])
    assert {k: v for k, v in fresh["param_groups"][0].items() if k != "params"} == {
        k: v for k, v in plain["param_groups"][0].items() if k != "params"}
    # HeadAdamW -> AdamW: the next torch step from the loaded state equals the next step of the original
    back = torch.optim.AdamW(params, lr=1e-3)
    back.load_state_dict(got)
    assert all(float(back.state[p]["step"]) == 2.0 for p in params)
    for p in params:
        assert torch.equal(back.state[p]["exp_avg"], ref.state[p]["exp_avg"])
        assert torch.equal(back.state[p]["exp_avg_sq"], ref.state[p]["exp_avg_sq"])


def test_load_state_dict_needs_equal_steps():
    params = _params()
    ref = torch.optim.AdamW(params)
    for p in params:
        p.grad = torch.ones_like(p)
    ref.step()
    params[0].grad = None
    ref.step()                                                            # the first parameter is one step behind
    with pytest.raises(ValueError, match="one step counter"):
        _HostAdamW(params).load_state_dict(ref.state_dict())


def test_refused_load_leaves_the_optimizer_as_it_was():
    params = _params()
    ref = torch.optim.AdamW(params, lr=5e-2, amsgrad=True)
    for p in params:
        p.grad = torch.ones_like(p)
    ref.step()
    host = _HostAdamW(params, lr=1e-3)
    before = host.state_dict()
    sd = ref.state_dict()
    for v in sd["state"].values():                                        # the state alone would load; the group must not
        del v["max_exp_avg_sq"]
    with pytest.raises(ValueError, match="amsgrad"):
        host.load_state_dict(sd)
    after = host.state_dict()
    assert after["state"] == {} == before["state"] and after["param_groups"] == before["param_groups"]
    assert host.param_groups[0]["lr"] == 1e-3 and host.step_count() == 0 and not host.state


def test_constructor_refusals():
    from athd.optim import HeadAdamW
    cpu = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="CUDA"):
        HeadAdamW(cpu)
    with pytest.raises(ValueError, match="float32"):
        HeadAdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="one parameter group"):
        HeadAdamW([{"params": cpu}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(fused=True), dict(fused=False),
               dict(foreach=True), dict(foreach=False)):
        with pytest.raises(ValueError, match="does not support"):
            HeadAdamW(cpu, **kw)
    assert HeadAdamW.fused_clip is True


def test_workspace_bytes_and_limits():
    """host arithmetic of athd_head_step_workspace_bytes: 8 bytes per chunk of 4096 elements of each tensor, at most 64
    tensors and 4096 chunks (every update workgroup adds all partials, so the limit bounds that sum)"""
    from athd import native
    t = lambda *ns: native.step_table([(16, 16, 16, 16, n) for n in ns])
    assert native.head_step_workspace_bytes(t(1)) == 8
    assert native.head_step_workspace_bytes(t(*R.SIZES)) == 8 * sum(-(-n // 4096) for n in R.SIZES)
    assert native.head_step_workspace_bytes(t(*[5] * 64)) == 64 * 8
    assert native.head_step_workspace_bytes(t(*[5] * 65)) == 0
    assert native.head_step_workspace_bytes(t(5, 0)) == 0
    assert native.head_step_workspace_bytes(t(4096 * 4096)) == 4096 * 8
    assert native.head_step_workspace_bytes(t(4096 * 4096 + 1)) == 0
    assert native.head_step_workspace_bytes(t(4096 * 4095, 4097)) == 0
