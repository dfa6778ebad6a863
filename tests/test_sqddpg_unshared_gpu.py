"""SQDDPG and FACMADDPG with ``shared_params: False`` on the GPU under FLEX_UNSHARED_CRITICS=1.

csrc/sqddpg_unshared.hip (nets.sqddpg_shapley_unshared: forward, backward, the z_shared node) against the fp64 composition of
one critic per agent with distinct random weights, on tests/fp64_budget.py's error budget, at the smallest shapes at which the
work map (chunks of whole samples of one agent, 32-row tiles, a persistent backward grid per agent) can go wrong; the agents'
separation; determinism; the shared kernel on the same inputs when every critic holds one set of weights; the reference's own
modules (tests/golden/sqddpg_unshared3_*, facmaddpg_unshared3_*); the switch's rules; memory as a condition; FACMADDPG's four
loss modes against the per-agent loop; a short training run each."""
import functools
import os
import types
import warnings

import numpy as np
import pytest
import torch as th
import torch.nn as nn
import torch.nn.functional as F

from . import fp64_budget as fb
from .golden_io import G, StubEnv, _np, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors
from .sqddpg_unshared_floor import vector_sum_floors
from .test_sqddpg_unshared_cpu import FAC, ROLES, SQ, SWITCH, fac_state_dict, replay, sq_state_dict

pytestmark = pytest.mark.gpu

OBS = 5                       # observation columns per agent: an odd fc1 pitch, so the in-place column reads are unaligned
# (n, a, ns, b, layernorm).  Samples per chunk: spc = min(64, 256 // ns) = 64, 64, 25 for ns = 1, 3, 10.
CASES = [
    (1, 1, 1, 5, True),       # one agent, one coalition, b below one chunk, a part-filled tile
    (3, 1, 3, 64, False),     # odd n a = 3 (the (n a + 1) & ~1 rounding); b exactly spc, 192 rows = six full tiles
    (5, 1, 10, 26, True),     # odd n a = 5; b = spc + 1: a chunk of 250 rows (no multiple of 32) and one of a single sample
    (8, 4, 10, 25, True),     # n a = 32, the edge; b exactly spc
    (3, 4, 3, 65, False),     # b = spc + 1 at spc = 64
    (5, 4, 10, 7, False),     # the golden configuration's shape below one chunk, without LayerNorm
    (2, 1, 1, 16385, True),   # 257 chunks against an agent's backward grid of at most 256 wavefronts: the grid-stride loop;
]                             # and the only case from WGRAD_MIN_ROWS samples: z_shared's gradients through flexnet_wgrad_batched


@pytest.fixture(autouse=True)
def _switch_on(monkeypatch):
    monkeypatch.setenv(SWITCH, "1")


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _case.cache_clear()
    th.cuda.empty_cache()


def make_critics(n, a, layernorm, seed, same=False, hid=64, agent_id=True, obs=OBS):
    """One MLPCritic per agent on rows [obs_1 .. obs_n | n action blocks | onehot(i)], every parameter 0.2 randn."""
    from safe_marl_amd.nets import MLPCritic
    args = types.SimpleNamespace(hid_size=hid, layernorm=layernorm, hid_activation="relu", agent_id=agent_id)
    th.manual_seed(seed)
    cs = [MLPCritic(n * obs + n * a + n, 1, args) for _ in range(n)]
    with th.no_grad():
        for c in cs:
            for p in c.parameters():
                p.copy_(0.2 * th.randn_like(p))
    if same:
        for c in cs[1:]:
            c.load_state_dict(cs[0].state_dict())
    return nn.ModuleList(cs)


def draw_inputs(n, a, ns, b, seed, obs=OBS):
    g = th.Generator().manual_seed(seed)
    o = 0.5 * th.randn(b, n, obs, generator=g)
    act = th.rand(b, n, a, generator=g)
    pos = th.argsort(th.rand(b * ns, n, generator=g), dim=1).argsort(dim=1)
    w = th.randn(b, n, generator=g) / b                      # upstream of phi
    u = th.randn(b, ns, n, generator=g) / (b * ns)           # upstream of q
    return o, act, pos, w, u


def coalition_rows(obs, act, pos, ns):
    """sqddpg.py:63-104's rows [b, ns, n, w] (fb.sqddpg_plain's construction): only agent i's own action keeps its gradient."""
    b, n, a = act.shape
    dev = act.device
    pos = pos.long().view(b, ns, n)
    who = th.empty_like(pos).scatter_(2, pos, th.arange(n, device=dev).expand(b, ns, n))
    ordered = act.unsqueeze(1).expand(b, ns, n, a).gather(2, who.unsqueeze(-1).expand(b, ns, n, a)).unsqueeze(2)
    p = th.arange(n, device=dev).view(1, 1, 1, n)
    own = (p == pos.unsqueeze(-1)).to(act.dtype).unsqueeze(-1)
    before = (p < pos.unsqueeze(-1)).to(act.dtype).unsqueeze(-1)
    acts = ordered.detach() * before + ordered * own
    return th.cat((obs.reshape(b, 1, 1, -1).expand(b, ns, n, -1), acts.reshape(b, ns, n, n * a),
                   th.eye(n, dtype=act.dtype, device=dev).expand(b, ns, n, n)), -1)


def plain(critics, obs, act, pos, ns):
    """Row (b, s, i) through critic i: (phi [b, n], q [b, ns, n], per agent (z1, first ReLU's pre-activation, second ReLU's) of
    its b ns rows)."""
    b, n, _ = act.shape
    rows = coalition_rows(obs, act, pos, ns)
    qs, pres = [], []
    for i, c in enumerate(critics):
        z1 = F.linear(rows[:, :, i].reshape(b * ns, -1), c.fc1.weight, c.fc1.bias)
        q, pre1, pre2 = fb.critic_tail_plain(c, z1)
        qs.append(q.view(b, ns))
        pres.append((z1, pre1, pre2))
    q = th.stack(qs, -1)
    return q.mean(1), q, pres


def loss_of(phi, q, w, u, keep, with_q):
    """tests/test_sqddpg_gpu.py's loss, and an upstream gradient of q when the rows' values are asked for."""
    loss = (phi * w).sum() + 0.1 * ((phi.sum(-1) ** 2) * keep).mean()
    return loss + (q * u).sum() if with_q else loss


def tied_pairs(c64, obs, act, pos, ns):
    """[b, n] bool: agent i of sample b has a coalition row with a ReLU pre-activation within 1e-5 of zero in fp64."""
    b, n, _ = act.shape
    with th.no_grad():
        pres = plain(c64, obs.double(), act.double(), pos, ns)[2]
    return th.stack([fb.tie_rows(list(p[1:])).view(b, ns).any(1) for p in pres], 1)


def composition(critics, obs, act, pos, ns, w, u, keep, dtype, with_q):
    """(phi, q, {name: gradient}, {name: floor}): the gradients of the own actions, the observations and every parameter; the
    floors (the fp64 run's alone) are those of each critic's tail sums, fb.tail_sum_floors's addends in the order this kernel
    sums them (tests/sqddpg_unshared_floor.py says why, with the figures that missed the exchangeable form)."""
    a = act.detach().to(dtype).requires_grad_(True)
    o = obs.detach().to(dtype).requires_grad_(True)
    phi, q, pres = plain(critics, o, a, pos, ns)
    loss = loss_of(phi, q, w.to(dtype), u.to(dtype), keep.to(dtype), with_q)
    params = dict(critics.named_parameters())
    floors = {}
    if dtype == th.float64:
        b, n, _ = act.shape
        g_q = th.autograd.grad(loss, [q], retain_graph=True)[0]
        for i, (c, (z1, pre1, pre2)) in enumerate(zip(critics, pres)):
            g1, g2 = th.autograd.grad(loss, [pre1, pre2], retain_graph=True)
            fl = vector_sum_floors(g_q[:, :, i].reshape(-1, 1), g1, g2, pre1, pre2, c.layernorm if c.args.layernorm else None, ns)
            floors.update({f"{i}.{k}": v for k, v in fl.items()})
    grads = th.autograd.grad(loss, [a, o] + list(params.values()))
    return phi.detach(), q.detach(), dict(zip(["act", "obs"] + list(params), grads)), floors


def kernel(critics, obs, act, pos, ns, w, u, keep, with_q, frozen=False):
    from safe_marl_amd.nets import sqddpg_shapley_unshared
    b, n, _ = act.shape
    a = act.clone().requires_grad_(True)
    o = obs.reshape(b, -1).clone().requires_grad_(True)
    phi, q = sqddpg_shapley_unshared(critics, o, a, pos, ns, want_q=with_q, frozen=frozen)
    assert "SqddpgUnsharedFn" in type(phi.grad_fn).__name__
    params = {} if frozen else dict(critics.named_parameters())
    loss = loss_of(phi, q, w, u, keep, with_q)
    grads = th.autograd.grad(loss, [a, o] + list(params.values()))
    out = dict(zip(["act", "obs"] + list(params), grads))
    out["obs"] = out["obs"].view_as(obs)
    return phi.detach(), (q.detach() if with_q else None), out


@functools.lru_cache(maxsize=None)
def _case(n, a, ns, b, layernorm, same=False, attempts=32):
    """The first draw whose tie share is within fb.TIE_CAP (a condition on the inputs, found in fp64 before any kernel runs),
    the tied pairs' upstream cleared, and the fp32 and fp64 compositions with and without an upstream gradient of q."""
    for attempt in range(attempts):
        critics = make_critics(n, a, layernorm, seed=11 * n + a + 1000 * attempt, same=same).cuda()
        obs, act, pos, w, u = [t.cuda() for t in draw_inputs(n, a, ns, b, seed=100 * b + 10 * n + ns + 1000 * attempt)]
        c64 = fb.ref64(critics)
        tie = tied_pairs(c64, obs, act, pos, ns)
        if float(tie.double().mean()) <= fb.TIE_CAP:
            break
    else:
        raise AssertionError(f"no draw of {n}x{a} ns={ns} b={b} within the tie cap in {attempts} attempts")
    w[tie] = 0
    u.transpose(1, 2)[tie] = 0
    keep = (~tie.any(1)).float()
    refs = {wq: (composition(critics, obs, act, pos, ns, w, u, keep, th.float32, wq),
                 composition(c64, obs, act, pos, ns, w, u, keep, th.float64, wq)) for wq in (True, False)}
    return critics, obs, act, pos, w, u, keep, refs


def check_budget(tag, got, t32, r64):
    phi, q, grads = got
    for nm, g, k in (("phi", phi, 0), ("q", q, 1)):
        if g is not None:
            assert th.isfinite(g).all(), (tag, nm)
            fb.within_budget(g, t32[k], r64[k], name=f"{tag} {nm}")
    for nm, g in grads.items():
        assert th.isfinite(g).all(), (tag, nm)
        fb.within_budget(g, t32[2][nm], r64[2][nm], floor_ulps=fb.floor_ulps(r64[3].get(nm), r64[2][nm]), name=f"{tag} d_{nm}")


@pytest.mark.parametrize("n,a,ns,b,layernorm", CASES)
def test_forward_and_backward_within_budget(n, a, ns, b, layernorm):
    """Every output and every gradient — d_act_own, d_z_shared (through the observations' gradient, fc1.bias and fc1.weight's
    observation columns), the action and id columns of every fc1.weight, every tail — with d_q given and NULL, with and without
    parameter gradients."""
    from safe_marl_amd import util
    critics, obs, act, pos, w, u, keep, refs = _case(n, a, ns, b, layernorm)
    before = dict(util.FALLBACKS)
    tag = f"sqddpg_unshared {n}x{a} ns={ns} b={b} ln={int(layernorm)}"
    with_dq = kernel(critics, obs, act, pos, ns, w, u, keep, True)
    assert set(with_dq[2]) == set(refs[True][1][2])
    check_budget(tag + " d_q", with_dq, *refs[True])
    no_dq = kernel(critics, obs, act, pos, ns, w, u, keep, False)
    check_budget(tag, no_dq, *refs[False])
    assert th.equal(no_dq[0], with_dq[0])                                      # phi does not depend on whether q is asked for
    # frozen (a policy sub-update): the kernel without parameter gradients gives the same bits for what it still writes
    fr = kernel(critics, obs, act, pos, ns, w, u, keep, False, frozen=True)
    assert set(fr[2]) == {"act", "obs"}
    assert th.equal(fr[0], no_dq[0]) and th.equal(fr[2]["act"], no_dq[2]["act"]) and th.equal(fr[2]["obs"], no_dq[2]["obs"])
    # critic i's id columns k != i never meet a 1: exactly zero, as autograd of the composition gives
    no = n * OBS + n * a
    for i in range(n):
        gid, rid = with_dq[2][f"{i}.fc1.weight"][:, no:], refs[True][1][2][f"{i}.fc1.weight"][:, no:]
        for k in range(n):
            if k != i:
                assert th.count_nonzero(gid[:, k]) == 0 and th.count_nonzero(rid[:, k]) == 0, (i, k)
    assert util.FALLBACKS == before


def test_each_output_alone_gives_the_bits_of_both():
    """phi only, q only and both through the entry point itself."""
    from safe_marl_amd import _lib, nets
    n, a, ns, b = 3, 4, 3, 65
    critics, obs, act, pos, *_ = _case(n, a, ns, b, False)
    flat = []
    for c in critics:
        flat += [c.fc1.weight, *nets._tail_params(c)[:-1]]
    ps = [flat[7 * i:7 * (i + 1)] for i in range(n)]
    with th.no_grad():
        z = nets._SqddpgZSharedFn.apply(obs.reshape(b, -1), n * OBS, *[t for c in critics for t in (c.fc1.weight, c.fc1.bias)])
    pos32 = pos.to(th.int32).contiguous()
    outs = {}
    for want in ("both", "phi", "q"):
        phi = th.full((b, n), float("nan"), device="cuda")
        q = th.full((b, ns, n), float("nan"), device="cuda")
        k = nets._sqddpg_unshared_args(z.contiguous(), act, pos32, ns, 1e-5, False, n * OBS, ps)
        if want != "q":
            k.phi = phi.data_ptr()
        if want != "phi":
            k.q = q.data_ptr()
        _lib.launch("flexnet_sqddpg_unshared_forward", k)
        outs[want] = (phi, q)
    assert th.equal(outs["phi"][0], outs["both"][0]) and th.equal(outs["q"][1], outs["both"][1])
    assert th.isnan(outs["phi"][1]).all() and th.isnan(outs["q"][0]).all()       # the output not asked for is not touched
    assert th.isfinite(outs["both"][0]).all() and th.isfinite(outs["both"][1]).all()


def test_agents_are_separate():
    from safe_marl_amd.nets import sqddpg_shapley_unshared
    n, a, ns, b = 3, 4, 3, 65
    critics, obs, act, pos, w, u, keep, refs = _case(n, a, ns, b, False)
    o2 = obs.reshape(b, -1)
    names = [k for k, _ in critics.named_parameters()]
    for j in range(n):                                                         # d_phi zero except agent j
        phi, _ = sqddpg_shapley_unshared(critics, o2, act, pos, ns)
        grads = th.autograd.grad((phi[:, j] * w[:, j]).sum(), list(critics.parameters()), allow_unused=True)
        for k, g in zip(names, grads):
            if int(k.split(".")[0]) == j:
                assert g is not None and th.count_nonzero(g) > 0, (j, k)
            else:
                assert g is None or th.count_nonzero(g) == 0, (j, k)           # exactly 0.0
    # swapping two critics: their agents' rows now return the other critic's values (the composition's, on the budget); the
    # third agent's are the same bits
    swapped = nn.ModuleList([critics[1], critics[0], critics[2]])
    with th.no_grad():
        phi, q = sqddpg_shapley_unshared(critics, o2, act, pos, ns, want_q=True)
        phi_s, q_s = sqddpg_shapley_unshared(swapped, o2, act, pos, ns, want_q=True)
        t32 = plain(swapped, obs, act, pos, ns)
        r64 = plain(fb.ref64(swapped), obs.double(), act.double(), pos, ns)
    fb.within_budget(phi_s, t32[0], r64[0], name="sqddpg_unshared swapped phi")
    fb.within_budget(q_s, t32[1], r64[1], name="sqddpg_unshared swapped q")
    assert th.equal(phi_s[:, 2], phi[:, 2]) and th.equal(q_s[:, :, 2], q[:, :, 2])
    assert not th.equal(phi_s[:, 0], phi[:, 0]) and not th.equal(phi_s[:, 1], phi[:, 1])


def test_two_calls_give_the_same_bits():
    n, a, ns, b, ln = 5, 1, 10, 26, True
    critics, obs, act, pos, w, u, keep, _ = _case(n, a, ns, b, ln)
    big = _case(2, 1, 1, 16385, True)                                          # the persistent grid with a second pass
    for cs, o, ac, p, ww, uu, kk, nss in ((critics, obs, act, pos, w, u, keep, ns), big[:7] + (1,)):
        x = kernel(cs, o, ac, p, nss, ww, uu, kk, True)
        y = kernel(cs, o, ac, p, nss, ww, uu, kk, True)
        assert th.equal(x[0], y[0]) and th.equal(x[1], y[1])
        assert all(th.equal(x[2][k], y[2][k]) for k in x[2])


@pytest.mark.parametrize("n,a,ns,b,layernorm", [(3, 4, 3, 65, True), (5, 4, 10, 26, False)])
def test_one_set_of_weights_agrees_with_the_shared_kernel(n, a, ns, b, layernorm):
    """All n critics holding one set of weights: phi / q and the per-agent gradients summed over the agents against
    flexnet_sqddpg_forward / _backward on the same inputs — both held to the one budget (whether they are in fact bit-equal is
    printed, not required).  A summed vector gradient's floor is the sum of the agents' floors."""
    from safe_marl_amd.nets import sqddpg_shapley_fused
    critics, obs, act, pos, w, u, keep, refs = _case(n, a, ns, b, layernorm, True)
    t32, r64 = refs[True]
    got = kernel(critics, obs, act, pos, ns, w, u, keep, True)
    a_ = act.clone().requires_grad_(True)
    o_ = obs.reshape(b, -1).clone().requires_grad_(True)
    phi_s, q_s = sqddpg_shapley_fused(critics[0], o_, a_, pos, ns, want_q=True)
    shared_params = dict(critics[0].named_parameters())
    gs = dict(zip(["act", "obs"] + list(shared_params),
                  th.autograd.grad(loss_of(phi_s, q_s, w, u, keep, True), [a_, o_] + list(shared_params.values()))))
    gs["obs"] = gs["obs"].view_as(obs)
    tag = f"sqddpg_unshared same-weights {n}x{a} ns={ns} b={b}"
    for nm, mine, theirs, k in (("phi", got[0], phi_s.detach(), 0), ("q", got[1], q_s.detach(), 1)):
        fb.within_budget(mine, t32[k], r64[k], name=f"{tag} {nm} (per-agent kernel)")
        fb.within_budget(theirs, t32[k], r64[k], name=f"{tag} {nm} (shared kernel)")
        print(f"{tag} {nm}: bit-equal {th.equal(mine, theirs)}, max |diff| {float((mine - theirs).abs().max()):.3e}")
    for nm in ("act", "obs"):
        fb.within_budget(got[2][nm], t32[2][nm], r64[2][nm], name=f"{tag} d_{nm} (per-agent kernel)")
        fb.within_budget(gs[nm], t32[2][nm], r64[2][nm], name=f"{tag} d_{nm} (shared kernel)")
        print(f"{tag} d_{nm}: bit-equal {th.equal(got[2][nm], gs[nm])}")
    for nm in shared_params:
        total = lambda d: sum(d[f"{i}.{nm}"] for i in range(n))                # noqa: E731
        floor = sum(r64[3][f"{i}.{nm}"] for i in range(n)) if f"0.{nm}" in r64[3] else None
        ref = total(r64[2])
        fl = fb.floor_ulps(floor, ref)
        fb.within_budget(total(got[2]), total(t32[2]), ref, floor_ulps=fl, name=f"{tag} sum_i d_{nm} (per-agent kernel)")
        fb.within_budget(gs[nm], total(t32[2]), ref, floor_ulps=fl, name=f"{tag} d_{nm} (shared kernel)")
        print(f"{tag} d_{nm}: bit-equal {th.equal(total(got[2]), gs[nm])}")


# ---- the reference's own modules, through SQDDPG on the GPU ------------------------------------------------------------------------
def _tiled_pos(gold, key, args, tile):
    p = th.from_numpy(gold[key]).cuda()
    n, ns = args.agent_num, args.sample_size
    return p.view(-1, ns, n).repeat(tile, 1, 1).view(-1, n)


def _no_sqddpg_fallbacks(util):
    return "sqddpg" not in util.FALLBACKS and "sqddpg_unshared" not in util.FALLBACKS


@pytest.mark.parametrize("tile", [1, 64])
def test_kernel_path_matches_the_reference(tile):
    """tests/test_sqddpg_gpu.py's tolerances for the shared fixtures; tile 64: 2 048 samples, z_shared's gradients through
    flexnet_wgrad_batched (every loss is a mean over samples: invariant under tiling)."""
    from safe_marl_amd import learner, util
    util.FALLBACKS.pop("sqddpg", None)
    util.FALLBACKS.pop("sqddpg_unshared", None)
    args = golden_args(SQ, cuda=True)
    gold = golden_vectors(SQ)
    m = golden_model("SQDDPG", args, sq_state_dict(device="cuda"), "cuda")
    b = golden_batch(SQ, "cuda", tile)
    n = args.agent_num
    calls = []
    real = learner.sqddpg_shapley_unshared
    learner.sqddpg_shapley_unshared = lambda *a_, **k: (calls.append(1), real(*a_, **k))[1]
    try:
        src = {}
        m.coalition_source = lambda role, groups: src[role]
        src["value"] = _tiled_pos(gold, "pos.call.value", args, tile)
        with th.no_grad():
            v = m.value(b.state, b.action)
            assert np.allclose(_np(v)[:32], gold["value"], atol=2e-5), np.abs(_np(v)[:32] - gold["value"]).max()
            phi = v.mean(1).view(-1, n)
            assert np.allclose(_np(phi)[:32], gold["phi"], atol=2e-5)
            assert np.allclose(_np(phi.sum(-1))[:32], gold["S"], atol=1e-4)
            src["target"] = _tiled_pos(gold, "pos.call.target", args, tile)
            _, na, _, _, _ = m.get_actions(b.next_state, status="train", exploration=False, actions_avail=b.action_avail,
                                           target=False, last_hid=b.hid)
            nphi, _ = m.target_net.shapley_values(b.next_state, na, src["target"])
            assert np.allclose(_np(nphi.sum(-1))[:32], gold["S_next"], atol=1e-4)
        assert len(calls) == 2
        src.update({r: _tiled_pos(gold, f"pos.loss.{r}", args, tile) for r in ROLES})
        pl, vl, _ = m.get_loss(b)
        assert len(calls) == 5
        assert abs(pl.item() - float(gold["policy_loss"])) < 1e-5
        assert abs(vl.item() - float(gold["value_loss"])) < 1e-4 * max(1.0, abs(float(gold["value_loss"])))
        for k, g in zip([k for k, _ in m.value_dicts.named_parameters()],
                        th.autograd.grad(vl, list(m.value_dicts.parameters()), retain_graph=True)):
            r = gold["vgrad." + k]
            assert np.allclose(_np(g), r, atol=2e-6 + 2e-4 * np.abs(r).max()), (tile, k, np.abs(_np(g) - r).max())
        for k, g in zip([k for k, _ in m.policy_dicts.named_parameters()], th.autograd.grad(pl, list(m.policy_dicts.parameters()))):
            r = gold["pgrad." + k]
            assert np.allclose(_np(g), r, atol=2e-7 + 2e-4 * np.abs(r).max()), (tile, k, np.abs(_np(g) - r).max())
        _, vl2, _ = m.get_loss(b, need="value")
        assert abs(vl2.item() - vl.item()) < 1e-5 * max(1.0, abs(vl.item()))
        pl2, _, _ = m.get_loss(b, need="policy")
        assert abs(pl2.item() - pl.item()) < 1e-6
    finally:
        learner.sqddpg_shapley_unshared = real
    assert _no_sqddpg_fallbacks(util)


def test_trainer_steps_and_target_update_match_the_reference():
    from safe_marl_amd import util
    from safe_marl_amd.learner import SQDDPG
    from safe_marl_amd.trainer import PGTrainer
    util.FALLBACKS.pop("sqddpg", None)
    util.FALLBACKS.pop("sqddpg_unshared", None)
    args = golden_args(SQ, cuda=True)
    gold = golden_vectors(SQ)
    tr = PGTrainer(args, SQDDPG, StubEnv(args.agent_num), None)
    sd = sq_state_dict(device="cuda")
    tr.behaviour_net.load_state_dict(sd)
    tr.behaviour_net.target_net.load_state_dict({k[len("target_net."):]: v for k, v in sd.items() if k.startswith("target_net.")})
    b = golden_batch(SQ, "cuda")
    stat = {}
    replay(tr.behaviour_net, gold, "vstep", device="cuda")
    tr.value_transition_process(stat, b)
    replay(tr.behaviour_net, gold, "pstep", device="cuda")
    tr.policy_transition_process(stat, b)
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_value_grad_norm", "mean_train_policy_grad_norm"):
        ref = gold["stat." + k]
        assert abs(float(stat[k]) - ref) < 2e-4 * max(1.0, abs(ref)), k
    cur = tr.behaviour_net.state_dict()
    for k, v in sq_state_dict("state_dict_after_step", "cuda").items():
        assert np.allclose(_np(cur[k]), _np(v), atol=5e-5), (k, np.abs(_np(cur[k]) - _np(v)).max())
    tr.behaviour_net.update_target()
    cur = tr.behaviour_net.target_net.state_dict()
    for k, v in golden_tensors(f"{SQ}_target_after_update.npz", "cuda").items():
        assert np.allclose(_np(cur[k]), _np(v), atol=5e-5), k
    assert _no_sqddpg_fallbacks(util)


# ---- the switch ---------------------------------------------------------------------------------------------------------------------
def _cpu_phi(m, args, b, pos):
    from safe_marl_amd.learner import SQDDPG
    mc = SQDDPG(args._replace(cuda=False))
    mc.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    return mc.shapley_values(b.state.cpu(), b.action.cpu(), pos.cpu())[0].detach().numpy()


def test_unset_the_call_is_the_composition_with_its_note(monkeypatch):
    from safe_marl_amd import util
    from safe_marl_amd.learner import SQDDPG
    monkeypatch.delenv(SWITCH)
    args = golden_args(SQ, cuda=True)
    th.manual_seed(0)
    m = SQDDPG(args).cuda()
    b = golden_batch(SQ, "cuda")
    pos = th.from_numpy(golden_vectors(SQ)["pos.call.value"]).cuda()
    util.FALLBACKS.pop("sqddpg", None)
    util.FALLBACKS.pop("sqddpg_unshared", None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        phi, _ = m.shapley_values(b.state, b.action, pos)
    assert util.FALLBACKS.get("sqddpg", 0) == 1 and "sqddpg_unshared" not in util.FALLBACKS
    assert phi.grad_fn is None or "SqddpgUnsharedFn" not in type(phi.grad_fn).__name__
    assert np.allclose(_np(phi), _cpu_phi(m, args, b, pos), atol=2e-5)
    # the same call with the switch set takes the kernel: no note of either family
    monkeypatch.setenv(SWITCH, "1")
    util.FALLBACKS.pop("sqddpg", None)
    phi2, _ = m.shapley_values(b.state, b.action, pos)
    assert "SqddpgUnsharedFn" in type(phi2.grad_fn).__name__ and _no_sqddpg_fallbacks(util)
    assert np.allclose(_np(phi2), _np(phi), atol=2e-5)
    with warnings.catch_warnings():                                           # _fused keeps its meaning and its note
        warnings.simplefilter("ignore")
        assert not m._fused(b.action)
    assert util.FALLBACKS.get("sqddpg", 0) == 1


@pytest.mark.parametrize("over", [dict(hid_size=32), dict(agent_id=False)])
def test_set_with_a_declined_configuration_notes_it_and_runs_the_composition(over):
    from safe_marl_amd import util
    from safe_marl_amd.learner import SQDDPG
    args = golden_args(SQ, cuda=True, **over)
    th.manual_seed(0)
    m = SQDDPG(args).cuda()
    b = golden_batch(SQ, "cuda")
    pos = th.from_numpy(golden_vectors(SQ)["pos.call.value"]).cuda()
    util.FALLBACKS.pop("sqddpg", None)
    util.FALLBACKS.pop("sqddpg_unshared", None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        phi, _ = m.shapley_values(b.state, b.action, pos)
    assert util.FALLBACKS.get("sqddpg_unshared", 0) == 1 and "sqddpg" not in util.FALLBACKS
    assert np.allclose(_np(phi), _cpu_phi(m, args, b, pos), atol=2e-5)


# ---- memory, as a condition -----------------------------------------------------------------------------------------------------------
def test_forward_and_backward_stay_far_below_the_materialised_rows():
    """b = 4096, ns = 10, n = 5, w = 745: the rows alone are b ns n w 4 bytes = 610 MB per term, and any path that forms them
    exceeds that.  The kernel path may hold a quarter above its inputs (obs, act, pos, the parameters); what it does hold —
    z_shared and its gradient, the parameter-gradient workspace (dropped before the measurement, so that it is counted whatever
    ran before), q, the gradients — is a fraction of that."""
    from safe_marl_amd import nets, util
    from safe_marl_amd.learner import SQDDPG
    args = golden_args("sqddpg", cuda=True, shared_params=False)
    th.manual_seed(0)
    m = SQDDPG(args).cuda()
    B, ns, n, wdt = 4096, args.sample_size, args.agent_num, m.value_dicts[0].fc1.weight.shape[1]
    assert (ns, n, wdt) == (10, 5, 745)
    g = th.Generator(device="cuda").manual_seed(1)
    obs = th.randn(B, n, m.obs_dim, device="cuda", generator=g)
    act = th.rand(B, n, m.act_dim, device="cuda", generator=g)
    pos = th.argsort(th.rand(B * ns, n, device="cuda", generator=g), dim=1).argsort(dim=1).to(th.int32)
    (th.randn(64, 64, device="cuda") @ th.randn(64, 64, device="cuda")).sum().item()      # the BLAS library's own workspace
    util.FALLBACKS.pop("sqddpg_unshared", None)
    for key in [k for k in nets._SCRATCH if isinstance(k[0], tuple) and k[0][0] == "sqddpg_unshared"]:
        del nets._SCRATCH[key]                              # the persistent parameter-gradient workspace counts: allocate it anew
    th.cuda.synchronize()
    th.cuda.empty_cache()
    th.cuda.reset_peak_memory_stats()
    base = th.cuda.memory_allocated()
    phi, q = m.shapley_values(obs, act, pos, want_q=True)
    grads = th.autograd.grad((phi * phi).sum() + q.sum(), list(m.value_dicts.parameters()))
    th.cuda.synchronize()
    assert all(th.isfinite(t).all() for t in grads) and "sqddpg_unshared" not in util.FALLBACKS
    peak = th.cuda.max_memory_allocated() - base
    bound = B * ns * n * wdt * 4 // 4
    print(f"sqddpg_unshared peak above the inputs: {peak / 2 ** 20:.1f} MiB, bound {bound / 2 ** 20:.1f} MiB")
    assert peak < bound, (peak, bound)


# ---- FACMADDPG ------------------------------------------------------------------------------------------------------------------------
TILE = 64                     # 2 048 samples, 6 144 critic rows: from WGRAD_MIN_ROWS upward every graph-carrying value is the node's


def _fac_model(tile=TILE):
    args = golden_args(FAC, cuda=True)
    m = golden_model("FACMADDPG", args, fac_state_dict(device="cuda", target_mixer=True), "cuda")
    return args, m, golden_batch(FAC, "cuda", tile)


def _fac_grads(m, b, need):
    """(policy loss, value loss, {name: gradient}) of one get_loss call in mode ``need``: what each optimiser would take."""
    pl, vl, _ = m.get_loss(b, need=need)
    out = {}
    if need in ("value", "both"):
        ps = dict(m.value_dicts.named_parameters())
        out.update({"v." + k: g for k, g in zip(ps, th.autograd.grad(vl, list(ps.values()), retain_graph=True))})
    if need in ("mixer", "both"):
        ps = dict(m.mixer.named_parameters())
        out.update({"m." + k: g for k, g in zip(ps, th.autograd.grad(vl, list(ps.values()), retain_graph=True))})
    if need in ("policy", "both"):
        ps = dict(m.policy_dicts.named_parameters())
        out.update({"p." + k: g for k, g in zip(ps, th.autograd.grad(pl, list(ps.values())))})
    return pl, vl, out


@pytest.mark.parametrize("need", ["value", "mixer", "policy", "both"])
def test_facmaddpg_losses_and_gradients_against_the_loop(need, monkeypatch):
    """The switch set (csrc/critic_unshared.hip: the node where the values carry a graph, the no-grad launch for the targets and
    for the mixer's step) against the per-agent loop with it unset, in one process; tests/test_critic_unshared_golden_gpu.py's
    bounds: value gradients 2e-6 + 1e-4 max|loop|, losses 2e-4 relative, policy gradients 2e-4 of the tensor's largest entry."""
    from safe_marl_amd import learner, util
    args, m, b = _fac_model()
    nodes, launches = [], []
    real_train, real_forward = learner.critic_unshared_train, learner.fused_critic_forward_unshared
    monkeypatch.setattr(learner, "critic_unshared_train", lambda *a, **k: (nodes.append(1), real_train(*a, **k))[1])
    monkeypatch.setattr(learner, "fused_critic_forward_unshared", lambda *a, **k: (launches.append(1), real_forward(*a, **k))[1])
    declined = util.FALLBACKS.get("critic_unshared", 0)
    pl, vl, got = _fac_grads(m, b, need)
    assert len(nodes) == {"value": 1, "mixer": 0, "policy": 1, "both": 2}[need]
    assert len(launches) == {"value": 1, "mixer": 2, "policy": 0, "both": 1}[need]
    assert util.FALLBACKS.get("critic_unshared", 0) == declined
    monkeypatch.delenv(SWITCH)
    n_before = (len(nodes), len(launches))
    pl0, vl0, ref = _fac_grads(m, b, need)
    assert (len(nodes), len(launches)) == n_before                             # unset: the loop, no launch of the family
    if vl is not None:
        assert abs(vl.item() - vl0.item()) <= 2e-4 * max(1.0, abs(vl0.item()))
    if pl is not None:
        assert abs(pl.item() - pl0.item()) <= 1e-5 * max(1.0, abs(pl0.item()))
    assert set(got) == set(ref) and got
    for k, g in got.items():
        r = ref[k]
        err, scale = float((g - r).abs().max()), float(r.abs().max())
        bound = 2e-4 * scale if k.startswith("p.") else 2e-6 + 1e-4 * scale
        print(f"facmaddpg unshared {need} {k}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)


def test_facmaddpg_kernel_path_matches_the_reference():
    from safe_marl_amd import util
    args, m, b = _fac_model()
    gold = golden_vectors(FAC)
    mgold = dict(np.load(os.path.join(G, FAC + "_golden_mixer_grads.npz")))
    declined = util.FALLBACKS.get("critic_unshared", 0)
    with th.no_grad():
        v = m.value(b.state, b.action)
        assert np.allclose(_np(v)[:32], gold["value"], atol=2e-5)
    pl, vl, got = _fac_grads(m, b, "both")
    assert abs(vl.item() - float(gold["value_loss"])) <= 2e-4 * max(1.0, abs(float(gold["value_loss"])))
    assert abs(pl.item() - float(gold["policy_loss"])) <= 1e-5 * max(1.0, abs(float(gold["policy_loss"])))
    for k, g in got.items():
        want = {"v": gold.get("vgrad." + k[2:]), "m": mgold.get("mgrad." + k[2:]), "p": gold.get("pgrad." + k[2:])}[k[0]]
        err, scale = np.abs(_np(g) - want).max(), np.abs(want).max()
        bound = 2e-4 * scale if k[0] == "p" else 2e-6 + 1e-4 * scale
        assert err <= bound, (k, err, bound)
    assert util.FALLBACKS.get("critic_unshared", 0) == declined


# ---- a short training run each ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ["SQDDPG", "FACMADDPG"])
def test_short_training_run_moves_critic_and_policy(alg):
    from safe_marl_amd import learner, util
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    blds = [5, 10, 15, 20, 25]
    env_args = {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds}
    net = create_network(env_args)
    env = VecFlexProvisionEnv(env_args, 256, net=net, series=make_synthetic_series(net, n_days=60), seed=3, warm_start=True)
    args = golden_args(alg.lower(), cuda=True, agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size,
                       v_min=0.9, v_max=1.1, target_update_freq=60, value_update_epochs=2, shared_params=False)
    for k in ("sqddpg", "sqddpg_unshared", "critic_unshared"):
        util.FALLBACKS.pop(k, None)
    th.manual_seed(0)
    np.random.seed(0)
    tr = PGTrainer(args, getattr(learner, alg), env, None, batch_scale=64, replay_capacity=256 * 96 * 2)
    net_ = tr.behaviour_net
    c0 = [p.detach().clone() for p in net_.value_dicts.parameters()]
    p0 = [p.detach().clone() for p in net_.policy_dicts.parameters()]
    stat = {}
    for _ in range(2):
        net_.train_process(stat, tr)
    th.cuda.synchronize()
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_value_grad_norm"):
        assert k in stat and np.isfinite(float(stat[k])), k
    assert all(not th.equal(a, p) for a, p in zip(c0, net_.value_dicts.parameters()))
    assert any(not th.equal(a, p) for a, p in zip(p0, net_.policy_dicts.parameters()))
    assert not any(k in util.FALLBACKS for k in ("sqddpg", "sqddpg_unshared", "critic_unshared")), dict(util.FALLBACKS)
