"""tests/fp64_budget.py itself, on the CPU: its plain compositions are the modules' forward; every input family keeps the share
of rows with an arbitrary ReLU side within the cap; the fp32 modules pass their own budget; and the budget rejects four wrong
fp32 results — two of them (a gradient off by 1e-5 of itself, an output off by 1e-5 of its scale) errors that the fixed
tolerances of the fp32-against-fp32 tests accept."""
import pytest
import torch as th

from . import fp64_budget as fb

ROWS, N, OBS, ACT = 2565, 5, 144, 4
ACTOR_FAMILIES = ("plain", "reset", "offset", "saturated", "dead", "mixed")
Z_FAMILIES = ("plain", "reset", "offset", "constant", "dead", "mixed")


def _actor_case(name, seed=1):
    g = th.Generator().manual_seed(seed)
    fam = fb.families(ROWS, N, OBS, g)[name]
    agent = fb.apply_params(fb.make_agent(OBS, N, ACT), fam)
    up = [th.randn(ROWS, ACT, generator=g) / ROWS, th.randn(ROWS, 64, generator=g) / ROWS]
    return fam, agent, up


def _actor_runs(fam, agent, up, **wrong):
    """(the module's own forward, the plain fp32 composition, the fp64 reference): outputs and parameter gradients."""
    obs, hid = fam.inputs
    a64 = fb.ref64(agent)
    share = fb.clear_ties(a64, (obs.double(), hid.double(), N), up)
    x = fb.with_ids(obs, N)
    module = fb.run_with_grads(lambda: agent(x, hid)[::2], dict(agent.named_parameters()), up)
    plain = fb.run_with_grads(lambda: fb.actor_plain(agent, obs, hid, N, **wrong)[:2], dict(agent.named_parameters()), up)
    ref = fb.run_with_grads(lambda: fb.actor_plain(a64, obs.double(), hid.double(), N)[:2], dict(a64.named_parameters()),
                            [u.double() for u in up])
    return share, module, plain, ref


def _check(module, plain, ref, tag):
    for k, nm in enumerate(("means", "hidden")):
        fb.within_budget(module[0][k], plain[0][k], ref[0][k], name=f"{tag} {nm}")
    for nm, g64 in ref[1].items():
        fb.within_budget(module[1][nm], plain[1][nm], g64, name=f"{tag} d_{nm}")


def test_plain_compositions_are_the_modules_forward():
    g = th.Generator().manual_seed(0)
    agent = fb.make_agent(OBS, N, ACT).double()
    obs, hid = th.randn(35, OBS, generator=g).double(), th.randn(35, 64, generator=g).double()
    with th.no_grad():
        m, _, h = agent(fb.with_ids(obs, N), hid)
        pm, ph, _ = fb.actor_plain(agent, obs, hid, N)
        assert (m - pm).abs().max() < 1e-12 and (h - ph).abs().max() < 1e-12
        critic = fb.make_critic().double()
        z = th.randn(35, 64, generator=g).double()
        q, _ = critic.forward_from_hidden(z, need_hidden=False)
        assert th.equal(q, fb.critic_tail_plain(critic, z)[0])
        oc, ac = th.randn(7, N * OBS, generator=g).double(), th.randn(7, N * ACT, generator=g).double()
        rows = th.cat([th.cat((oc, th.eye(N).double()[i].expand(7, -1), ac), -1) for i in range(N)], 0).view(N, 7, -1)
        z1 = critic.fc1(rows.transpose(0, 1).reshape(7 * N, -1))
        assert (z1 - fb.critic_first_layer_plain(critic, oc, ac, N)).abs().max() < 1e-12


@pytest.mark.parametrize("name", ACTOR_FAMILIES)
def test_actor_family_tie_share_and_the_modules_own_budget(name):
    fam, agent, up = _actor_case(name)
    share, module, plain, ref = _actor_runs(fam, agent, up)
    print(f"tie share {name}: {share:.4%}")
    assert share <= fb.TIE_CAP
    assert all(th.isfinite(t).all() for t in module[0]) and all(th.isfinite(g).all() for g in module[1].values())
    if name == "dead":
        for nm in ("fc1.weight", "fc1.bias", "layernorm.weight"):
            assert not ref[1][nm].any() and not module[1][nm].any()
    _check(module, plain, ref, f"cpu-module {name}")


@pytest.mark.parametrize("name", Z_FAMILIES)
def test_critic_family_tie_share_and_the_modules_own_budget(name):
    g = th.Generator().manual_seed(2)
    fam = fb.families(ROWS, N, None, g)[name]
    critic = fb.apply_params(fb.make_critic(), fam)
    up = th.randn(ROWS, 1, generator=g)
    c64 = fb.ref64(critic)
    z = fam.inputs[0]
    share = fb.clear_ties(c64, (z.double(),), up)
    print(f"tie share {name}: {share:.4%}")
    assert share <= fb.TIE_CAP
    tail = lambda c: {k: p for k, p in c.named_parameters() if not k.startswith("fc1")}

    def run(c, zz, fn, u):
        zz = zz.clone().requires_grad_(True)
        return fb.run_with_grads(lambda: (fn(c, zz),), dict(z=zz, **tail(c)), [u])

    module = run(critic, z, lambda c, zz: c.forward_from_hidden(zz, need_hidden=False)[0], up)
    # (on the CPU the module and the plain composition are the same ATen calls: the budget holds with a ratio of 1)
    plain = run(critic, z, lambda c, zz: fb.critic_tail_plain(c, zz)[0], up)
    ref = run(c64, z.double(), lambda c, zz: fb.critic_tail_plain(c, zz)[0], up.double())
    if name == "dead":
        assert not ref[1]["z"].any() and not module[1]["z"].any()
    fb.within_budget(module[0][0], plain[0][0], ref[0][0], name=f"cpu-critic {name} q")
    for nm, g64 in ref[1].items():
        fb.within_budget(module[1][nm], plain[1][nm], g64, name=f"cpu-critic {name} d_{nm}")


@pytest.mark.parametrize("name", ["plain", "reset", "offset", "dead"])
def test_budget_rejects_a_gradient_and_an_output_off_by_1e_5(name):
    """(fc2's weight gradient: the one no family makes zero.  Not on saturated rows: there the fp32 module's own error on the
    hidden state is 1.5e-5 of its scale — gate pre-activations of several tens carry an absolute error of 1e-5 into gates that
    are not yet saturated — which is what the yardstick is relative for.)"""
    fam, agent, up = _actor_case(name)
    _, module, plain, ref = _actor_runs(fam, agent, up)
    g64 = ref[1]["fc2.weight"]
    fb.within_budget(module[1]["fc2.weight"], plain[1]["fc2.weight"], g64, name="unmutated d_fc2.weight")
    with pytest.raises(AssertionError):
        fb.within_budget(module[1]["fc2.weight"] * (1.0 + 1e-5), plain[1]["fc2.weight"], g64, name="mutant d_fc2.weight (1 + 1e-5)")
    for k, nm in enumerate(("means", "hidden")):
        if name == "reset" and nm == "hidden":
            continue                     # (all-zero inputs: the new hidden state is one row repeated, an fp32 error of 0 is no luck)
        scale = float(ref[0][k].abs().max())
        with pytest.raises(AssertionError):
            fb.within_budget(module[0][k] + 1e-5 * scale, plain[0][k], ref[0][k], name=f"mutant {nm} + 1e-5 scale")


@pytest.mark.parametrize("name", ["plain", "offset", "mixed"])
@pytest.mark.parametrize("wrong", [dict(ln_units=63), dict(drop_id_of=N - 1)], ids=["ln-mean-over-63", "last-agent-id-dropped"])
def test_budget_rejects_a_wrong_layernorm_count_and_a_dropped_id_column(name, wrong):
    fam, agent, up = _actor_case(name)
    _, good, mutant, ref = _actor_runs(fam, agent, up, **wrong)
    for k, nm in enumerate(("means", "hidden")):
        with pytest.raises(AssertionError):
            fb.within_budget(mutant[0][k], good[0][k], ref[0][k], name=f"mutant {list(wrong)[0]} {name} {nm}")
    with pytest.raises(AssertionError):
        fb.within_budget(mutant[1]["fc1.weight"], good[1]["fc1.weight"], ref[1]["fc1.weight"],
                         name=f"mutant {list(wrong)[0]} {name} d_fc1.weight")


@pytest.mark.parametrize("b,n,obs_dim,act", [(13, 5, 144, 4), (7, 3, 72, 2), (130, 8, 6, 8)])
@pytest.mark.parametrize("wrong", [dict(ln_units=63), dict(drop_id_of=-1)], ids=["ln-mean-over-63", "last-agent-id-dropped"])
def test_the_floor_of_saturated_rows_still_rejects_the_wrong_evaluations(b, n, obs_dim, act, wrong):
    """fb.gate_rounding, the one wider floor (the inference launch on saturated rows, tests/test_actor_fp64_gpu.py), at that
    test's shapes: the fp32 module stays within the widened budget on all three tensors, and the two wrong evaluations are
    rejected on the means and the hidden state, the tensors that carry the rounding the floor stands for."""
    rows = b * n
    g = th.Generator().manual_seed(rows + act)
    obs, hid = fb.families(rows, n, obs_dim, g)["saturated"].inputs
    noise = th.randn(rows, act, generator=g)
    agent = fb.make_agent(obs_dim, n, act)
    a64 = fb.ref64(agent)
    explore = lambda out: (out[0], out[1], th.tanh(out[0] + 0.75 * noise.to(out[0].dtype)))
    with th.no_grad():
        module = explore(agent(fb.with_ids(obs, n), hid)[::2])
        good = explore(fb.actor_plain(agent, obs, hid, n)[:2])
        mutant = explore(fb.actor_plain(agent, obs, hid, n, **wrong)[:2])
        ref = explore(fb.actor_plain(a64, obs.double(), hid.double(), n)[:2])
    wide = fb.gate_rounding(a64, obs.double(), hid.double(), n, noise, 0.75)
    for k, nm in enumerate(("means", "hidden", "action")):
        floor = fb.FLOOR_ULPS + float(wide[nm].max()) / (fb.ULP * float(ref[k].abs().max()))
        fb.within_budget(module[k], good[k], ref[k], floor_ulps=floor, name=f"cpu-module saturated {b}x{n} {nm}")
        if nm != "action":
            with pytest.raises(AssertionError):
                fb.within_budget(mutant[k], good[k], ref[k], floor_ulps=floor, name=f"mutant {list(wrong)[0]} saturated {b}x{n} {nm}")
