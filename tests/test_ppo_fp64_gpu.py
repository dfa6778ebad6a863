"""csrc/ppo.hip on the fp64 error budget of tests/fp64_budget.py: GAE (flexnet_ppo_gae through nets.ppo_gae, and through the C
entry point on ragged chains), the policy loss in both instantiations (fixed log-std, per-row log-stds) and the value loss,
against the plain composition evaluated in fp64 on the same fp32 numbers — at the shapes where flexnet_ppo_gae picks another
kernel or a scan tile ends, and on the input families of ``fb.gae_families`` / ``fb.policy_families`` / ``fb.value_families``
(done = 1 on rows that are no last step, episode ends on lanes 0 and 63 of a scan tile, suffix sums, a column of failure
rewards, actions on the mean, ratios clipped out, log-stds at either end of their range, ...).  Every case is drawn from a
CPU generator: tests/test_fp64_budget_cpu.py holds the families' conditions and the kink shares of these very cases.  What
needs no tolerance comes last: a NaN stays in its row.  The figures of a run are filed in profiles/fp64_error_budget.txt."""
import ctypes as C

import pytest
import torch as th

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

COEF = 2.0
# (rows, n, chain_stride): csrc/ppo.hip takes the lane kernel up to PPO_LANE_MAX_STEPS = 256 steps, or with at least
# PPO_LANE_MIN_CHAINS = 16 384 chains, and the wavefront scan otherwise
GAE_SHAPES = [(24, 3, 8),            # lane kernel, 3 steps
              (512, 8, 2),           # lane, exactly 256 steps
              (514, 3, 2),           # wave, 257 steps: four tiles and one lane
              (320, 5, 1),           # wave, five whole tiles
              (1000, 5, 1),          # wave, a last tile of 40
              (526336, 8, 2048),     # lane on 257-step chains: 16 384 chains
              (2, 5, 1)]             # the smallest batch a BatchNorm takes: unbiased factor 2
GAE_RAGGED = [(29, 3, 8),            # lane: chains 0 .. 4 have four steps, the others three
              (901, 3, 3)]           # wave: chain 0 has 301 steps, the others 300
GAE_TENSORS = ("reward_norm", "advantages", "advantages_norm")
# (rows, n, a); the last: one thread of the PPO_BLOCKS x 256 takes a second row
POLICY_SHAPES = [(1, 1, 2), (33, 3, 4), (65, 5, 8), (257, 8, 8), (300, 5, 3), (256 * 256 + 1, 2, 2)]
# (family, index into fb.LOG_STD_RANGES): only the ends depend on the range
POLICY_CASES = [(f, 0) for f in fb.POLICY_FAMILIES] + [("ends_min", 1), ("ends_max", 1)]
VALUE_SHAPES = sorted({(rows, n) for rows, n, _ in POLICY_SHAPES})


def gae_case(rows, n, stride, family):
    """The family's inputs on the CPU (seeded by the shape)."""
    return fb.gae_families(rows, n, stride, th.Generator().manual_seed(1000 * rows + 10 * stride + n))[family]


def _gae_forms(fam, n, stride, bn):
    """(fp64 reference, fp32 composition) of fb.gae_plain on the CPU, each with its own pair of modules."""
    out = []
    for dtype in (th.float64, th.float32):
        mods = (fb.bn_module(n, dtype, seed=1), fb.bn_module(n, dtype, seed=2)) if bn else (None, None)
        out.append(fb.gae_plain(*[x.to(dtype) for x in fam.inputs], fam.params["gamma"], fam.params["lam"], stride, *mods))
    return out


def _compare_gae(tag, got, t32, ref, bn):
    for name in GAE_TENSORS:
        fb.within_budget(got[name].cpu(), t32[name], ref[name], name=f"{tag} {name}")
    if bn:
        for key in ("reward_bn", "adv_bn"):
            for stat in ("running_mean", "running_var"):
                fb.within_budget(got[f"{key}.{stat}"].cpu(), t32[f"{key}.{stat}"], ref[f"{key}.{stat}"], name=f"{tag} {key}.{stat}")
            assert int(got[f"{key}.num_batches_tracked"]) == int(ref[f"{key}.num_batches_tracked"]) == 1


@pytest.mark.parametrize("family", fb.GAE_FAMILIES)
@pytest.mark.parametrize("rows,n,stride", GAE_SHAPES)
def test_gae(rows, n, stride, family):
    from safe_marl_amd.nets import ppo_gae
    from safe_marl_amd.util import FALLBACKS
    fam = gae_case(rows, n, stride, family)
    gamma, lam = fam.params["gamma"], fam.params["lam"]
    args = [x.cuda() for x in fam.inputs]
    for bn in (True, False):
        ref, t32 = _gae_forms(fam, n, stride, bn)
        mods = (fb.bn_module(n, device="cuda", seed=1), fb.bn_module(n, device="cuda", seed=2)) if bn else (None, None)
        before = FALLBACKS.get("ppo_gae", 0)
        rn, adv, advn = ppo_gae(*args, gamma, lam, stride, *mods)
        assert FALLBACKS.get("ppo_gae", 0) == before                                   # the kernels ran
        got = {"reward_norm": rn, "advantages": adv, "advantages_norm": advn}
        for key, m in zip(("reward_bn", "adv_bn"), mods):
            if m is not None:
                got.update({f"{key}.running_mean": m.running_mean, f"{key}.running_var": m.running_var,
                            f"{key}.num_batches_tracked": m.num_batches_tracked})
        _compare_gae(f"gae {family} {rows}x{n}/{stride} bn={int(bn)}", got, t32, ref, bn)
        if not bn:
            assert th.equal(rn, args[0]) and advn is adv


def _entry_point(fam, n, stride, mods):
    """flexnet_ppo_gae through the C entry point (the Python wrapper asks for whole steps): every output prefilled with NaN."""
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import _ppo_bn_args
    r, v, nv, done, last = (x.cuda().contiguous() for x in fam.inputs)
    rn, adv, advn = (th.full_like(r, float("nan")) for _ in range(3))
    ws = th.empty(_lib.FLEXNET_PPO_WS_FLOATS // 2, dtype=th.float64, device="cuda")
    a = _lib.FlexPpoGaeArgs()
    a.rows, a.chain_stride, a.n_agents, a.gamma, a.lambda_ = r.shape[0], stride, n, fam.params["gamma"], fam.params["lam"]
    a.reward, a.old_values, a.old_next_values, a.done, a.last_step = (x.data_ptr() for x in (r, v, nv, done, last))
    _ppo_bn_args(a.reward_bn, mods[0])
    _ppo_bn_args(a.adv_bn, mods[1])
    a.reward_norm, a.advantages, a.workspace, a.workspace_floats = rn.data_ptr(), adv.data_ptr(), ws.data_ptr(), 2 * ws.numel()
    if mods[1] is not None:
        a.advantages_norm = advn.data_ptr()
    _lib.check(_lib.load().flexnet_ppo_gae(C.byref(a), C.c_void_p(th.cuda.current_stream().cuda_stream)), "flexnet_ppo_gae")
    th.cuda.synchronize()
    return rn, adv, (advn if mods[1] is not None else adv)


@pytest.mark.parametrize("family", ["plain", "tile_edges", "open_sum", "mixed"])
@pytest.mark.parametrize("rows,n,stride", GAE_RAGGED)
def test_gae_entry_point_on_ragged_chains(rows, n, stride, family):
    """rows % chain_stride != 0: the chains differ in length by one step.  The reference is the literal per-chain loop
    (fb.gae_chain_loop) in fp64."""
    assert rows % stride != 0
    fam = gae_case(rows, n, stride, family)
    for bn in (True, False):
        ref, t32 = _gae_forms(fam, n, stride, bn)
        mods = (fb.bn_module(n, device="cuda", seed=1), fb.bn_module(n, device="cuda", seed=2)) if bn else (None, None)
        rn, adv, advn = _entry_point(fam, n, stride, mods)
        got = {"reward_norm": rn, "advantages": adv, "advantages_norm": advn}
        for name, t in got.items():
            assert not th.isnan(t).any(), f"{name}: an element was not written"
        for key, m in zip(("reward_bn", "adv_bn"), mods):
            if m is not None:
                got.update({f"{key}.running_mean": m.running_mean, f"{key}.running_var": m.running_var,
                            f"{key}.num_batches_tracked": m.num_batches_tracked})
        _compare_gae(f"gae-ragged {family} {rows}x{n}/{stride} bn={int(bn)}", got, t32, ref, bn)


@pytest.mark.parametrize("rows,n,stride", [(1000, 5, 1), (526336, 8, 2048)])
def test_gae_failure_column_batch_statistics(rows, n, stride):
    """The batch statistics of the failure family's reward columns, each column against ITSELF: with momentum 1 a module's
    running statistics are the batch mean and the unbiased batch variance, which csrc/flex_td.h forms in fp64 as
    ss / rows - mean^2 — a difference of two numbers of 4e4 for a variance of 2.5e-3 (|mean| / std = 4 000).  Column 0 is
    constant: its variance is exactly zero in every form."""
    from safe_marl_amd.nets import ppo_gae
    fam = gae_case(rows, n, stride, "failure")
    forms = []
    for dtype, dev in ((th.float64, "cpu"), (th.float32, "cpu"), (th.float32, "cuda")):
        bn = fb.bn_module(n, dtype, dev, seed=1)
        bn.momentum = 1.0
        if dev == "cuda":
            ppo_gae(*[x.cuda() for x in fam.inputs], fb.GAMMA, fb.LAM, stride, bn, None)
        else:
            fb.gae_plain(*[x.to(dtype) for x in fam.inputs], fb.GAMMA, fb.LAM, stride, bn, None)
        forms.append((bn.running_mean.cpu(), bn.running_var.cpu()))
    ref, t32, got = forms
    assert float(ref[1][0]) == 0.0 and float(got[1][0]) == 0.0 and float(got[0][0]) == fb.FAILURE_REWARD
    for j in range(n):
        for k, stat in enumerate(("mean", "var")):
            fb.within_budget(got[k][j:j + 1], t32[k][j:j + 1], ref[k][j:j + 1], name=f"gae failure {rows}x{n}/{stride} batch {stat} of column {j}")


# ---- the policy loss --------------------------------------------------------------------------------------------------------
def policy_case(rows, n, a, family, per_row, which_range):
    """(family with the kinks' advantages cleared, kink share) on the CPU (seeded by the shape)."""
    g = th.Generator().manual_seed(1000 * rows + 100 * n + 10 * a + int(per_row))
    fam = fb.policy_families(rows, n, a, g, per_row=per_row, log_std_range=fb.LOG_STD_RANGES[which_range])[family]
    share = fb.policy_clear_kinks(fam.inputs, fam.params["eps_clip"])
    return fam, share


def _policy_kernel(inputs, eps_clip, per_row):
    """{"loss", "ratio", "d_means", "d_log_stds"} through nets.ppo_policy_loss on the GPU."""
    from safe_marl_amd.nets import ppo_policy_loss
    from safe_marl_amd.util import FALLBACKS
    means, log_stds, actions, old, adv = (t.cuda() for t in inputs)
    m = means.clone().requires_grad_(True)
    ls = log_stds.clone().requires_grad_(True) if per_row else fb.fixed_log_stds(m, log_stds)
    before = FALLBACKS.get("ppo_policy_loss", 0)
    loss, ratio = ppo_policy_loss(m, ls, actions, old, adv, eps_clip)
    assert FALLBACKS.get("ppo_policy_loss", 0) == before                               # the kernel ran
    grads = th.autograd.grad(loss, [m, ls] if per_row else [m])
    out = {"loss": loss.detach(), "ratio": ratio, "d_means": grads[0]}
    if per_row:
        out["d_log_stds"] = grads[1]
    return out


def _held_loss(held, got, t32, ref, inputs, eps_clip, name):
    """``held`` (fb.within_budget or its rms form; for one number they differ in their factors alone); a loss that misses it is
    held with fb.policy_loss_rounding's floor on top — the loss is ONE number whose terms cancel, and the fp32 composition's can
    come out within a fraction of an ulp by luck — and says so."""
    try:
        return held(got, t32, ref, name=name)
    except AssertionError:
        pass
    extra = float(fb.policy_loss_rounding(inputs, eps_clip)) / (fb.ULP * max(float(ref.abs()), fb.TINY))
    base = 4.0 if held is fb.within_budget_rms else fb.FLOOR_ULPS
    print(f"fp64-budget {name}: over the plain budget, held to the policy_loss_rounding floor ({extra:.1f} ulps of the loss)")
    return held(got, t32, ref, floor_ulps=base + extra, name=name + " [loss-rounding floor]")


@pytest.mark.parametrize("family,which_range", POLICY_CASES)
@pytest.mark.parametrize("rows,n,a", POLICY_SHAPES)
@pytest.mark.parametrize("per_row", [False, True], ids=["fixed", "rows"])
def test_policy_loss(per_row, rows, n, a, family, which_range):
    fam, share = policy_case(rows, n, a, family, per_row, which_range)
    eps_clip = fam.params["eps_clip"]
    assert share <= fb.TIE_CAP
    ref = fb.policy_loss_plain(fam.inputs, eps_clip, th.float64, fixed=not per_row)
    t32 = fb.policy_loss_plain(fam.inputs, eps_clip, th.float32, fixed=not per_row)
    got = _policy_kernel(fam.inputs, eps_clip, per_row)
    lo, hi = fb.LOG_STD_RANGES[which_range]
    tag = f"policy-{'rows' if per_row else 'fixed'} {family}[{lo},{hi}] {rows}x{n}x{a}"
    held = fb.within_budget_rms if family in fb.POLICY_RMS else fb.within_budget
    for name, r in ref.items():
        if name == "loss":
            _held_loss(held, got[name].cpu(), t32[name], r, fam.inputs, eps_clip, f"{tag} {name}")
        else:
            held(got[name].cpu(), t32[name], r, name=f"{tag} {name}")
    if family in ("on_mean", "zero_adv", "clipped_out"):
        assert not ref["d_means"].any() and not got["d_means"].any()
    if family in ("zero_adv", "clipped_out") and per_row:
        assert not ref["d_log_stds"].any() and not got["d_log_stds"].any()
    if family == "zero_adv":
        assert float(got["loss"]) == 0.0
    if per_row:
        assert all(th.equal(got["d_log_stds"][:, i], got["d_log_stds"][:, 0]) for i in range(n))
    assert all(th.equal(got["d_means"][:, i], got["d_means"][:, 0]) for i in range(n))  # the sums over agents, to every agent


@pytest.mark.parametrize("per_row", [False, True], ids=["fixed", "rows"])
def test_policy_loss_keeps_a_nan_in_its_row(per_row):
    """A NaN in one row's means: the loss is NaN, that row's gradients are NaN, every other row's keep the bits of the run
    without it."""
    rows, n, a, bad = 65, 3, 4, 37
    fam, _ = policy_case(rows, n, a, "plain", per_row, 0)
    clean = _policy_kernel(fam.inputs, fb.POLICY_EPS, per_row)
    means = fam.inputs[0].clone()
    means[bad, 1, 2] = float("nan")
    got = _policy_kernel((means,) + tuple(fam.inputs[1:]), fb.POLICY_EPS, per_row)
    others = th.arange(rows) != bad
    assert th.isnan(got["loss"]) and th.isfinite(clean["loss"])
    for name in ("d_means", "d_log_stds") if per_row else ("d_means",):
        assert th.isnan(got[name][bad]).all(), name
        assert th.equal(got[name][others], clean[name][others]), name
    assert th.isnan(got["ratio"][bad]).all() and th.equal(got["ratio"][others], clean["ratio"][others])


# ---- the value loss ---------------------------------------------------------------------------------------------------------
def value_case(rows, n, family):
    fam = fb.value_families(rows, n, th.Generator().manual_seed(1000 * rows + n))[family]
    return fam, fb.value_keep(fam.inputs, fam.params["eps_clip"], fb.GAMMA)


@pytest.mark.parametrize("family", fb.VALUE_FAMILIES)
@pytest.mark.parametrize("rows,n", VALUE_SHAPES)
def test_value_loss(rows, n, family):
    from safe_marl_amd.nets import ppo_value_loss
    from safe_marl_amd.util import FALLBACKS
    fam, keep = value_case(rows, n, family)
    eps_clip = fam.params["eps_clip"]
    assert 1.0 - float(keep.double().mean()) <= fb.TIE_CAP
    ref = fb.value_loss_plain(fam.inputs, eps_clip, fb.GAMMA, COEF, th.float64)
    t32 = fb.value_loss_plain(fam.inputs, eps_clip, fb.GAMMA, COEF, th.float32)
    values, old, nv, rn, done = (t.cuda() for t in fam.inputs)
    v = values.clone().requires_grad_(True)
    before = FALLBACKS.get("ppo_value_loss", 0)
    loss, ret = ppo_value_loss(v, old, nv, rn, done, fb.GAMMA, eps_clip, COEF)
    assert FALLBACKS.get("ppo_value_loss", 0) == before                                # the kernel ran
    (gv,) = th.autograd.grad(loss, [v])
    tag = f"value {family} {rows}x{n}"
    fb.within_budget(loss.detach().cpu(), t32["loss"], ref["loss"], name=f"{tag} loss")
    fb.within_budget(ret.cpu(), t32["returns"], ref["returns"], name=f"{tag} returns")
    fb.within_budget(gv.cpu()[keep], t32["d_values"][keep], ref["d_values"][keep], name=f"{tag} d_values")
    # the constructed rows, exact in every form: the clipped branch keeps its gradient AT the boundary (clamp's range includes
    # its ends); a tie outside the range hands half of the gradient to the unclipped branch only, 0.5 (V - ret) = 0.25; with
    # eps_clip = 0 a value equal to the old one is inside the range and a tie: the whole gradient
    unit = rows * n / (2 * COEF)
    ref_g, got_g = ref["d_values"] * unit, gv.double().cpu() * unit
    if family != "eps0":
        for k in (0, 1, 2):
            assert th.allclose(got_g[k::16], ref_g[k::16], atol=1e-6, rtol=0)
        if family == "plain":
            assert th.allclose(ref_g[2::16], th.full_like(ref_g[2::16], 0.25))
    else:
        assert th.allclose(got_g[3::16], ref_g[3::16], atol=1e-6, rtol=0)
        e1 = (fam.inputs[0].double() - ref["returns"])[3::16]
        assert th.allclose(ref_g[3::16], e1)
