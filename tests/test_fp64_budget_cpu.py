"""tests/fp64_budget.py itself, on the CPU: its plain compositions are the modules' forward; every input family — and every
case of the GPU tests that draw theirs from the CPU generator — keeps the share of rows with an arbitrary ReLU side within the
cap; the fp32 modules pass their own budget; and the budget rejects five wrong fp32 results — two of them (a gradient off by
1e-5 of itself, an output off by 1e-5 of its scale) errors that the fixed tolerances of the fp32-against-fp32 tests accept,
one (LayerNorm statistics from a running fp32 sum) wrong only on rows whose 64 inputs are all equal.  The QMIX mixer's part is
at the end: ``qmix_plain`` is ``QMixer.forward_torch``, every case of tests/test_qmix_fp64_gpu.py keeps its tie share within the
cap, and the budget rejects three wrong evaluations of the mixer.  The last part holds the cases of the two hand-written GEMMs
(tests/test_wgrad_fp64_gpu.py, tests/test_linear_fp64_gpu.py): a running fp32 sum in row (column) order is inside the budget with
the floors those tests take, and five wrong evaluations are outside it.  Then the optimiser step and the scalar mean
(tests/test_optim_fp64_gpu.py): ``clip_rmsprop_plain`` is the two PyTorch calls, its fp32 form and PyTorch's pass each other's budget
in every family, five wrong steps are outside it, and the bound of a mean rejects a sum held in fp32."""
import pytest
import torch as th

from . import fp64_budget as fb

ROWS, N, OBS, ACT = 2565, 5, 144, 4
ACTOR_FAMILIES = ("plain", "reset", "offset", "constant", "saturated", "dead", "mixed")
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


# ---------------------------------------------------------------------------------------------------------------------------
# the tile-scheme kernels' compositions, families and cases (tests/test_coma_fp64_gpu.py, test_sqddpg_fp64_gpu.py,
# test_critic_unshared_fp64_gpu.py, test_actor_mlp_fp64_gpu.py, test_unshared_fp64_gpu.py)

def test_tile_scheme_compositions_are_the_modules_forward():
    from safe_marl_amd.learner import SQDDPG
    from safe_marl_amd.nets import coma_baseline
    from .golden_io import golden_args
    g = th.Generator().manual_seed(0)
    n, o, a, b = 3, 30, 2, 7
    with th.no_grad():
        agent = fb.make_mlp_agent(o, n, a).double()
        obs = th.randn(b * n, o, generator=g).double()
        m, _, h = agent(fb.with_ids(obs, n), None)
        pm, ph, pre1, pre2 = fb.mlp_actor_plain(agent, obs, n)
        assert (m - pm).abs().max() < 1e-12 and (h - ph).abs().max() < 1e-12 and th.equal(th.relu(pre2), ph)
        one = fb.mlp_actor_plain(agent, obs[1::n], n, agent_index=1)            # every row agent 1: the per-agent modules' form
        assert (one[0] - pm[1::n]).abs().max() < 1e-12
        obs3, act3 = obs.view(b, n, o), th.randn(b, n, a, generator=g).double()
        for form, (shared, has_act) in fb.CRITIC_FORMS.items():
            width = o * (n if shared else 1) + n + (a * (n if shared else 1) if has_act else 0)
            critic = fb.make_critic(in_features=width).double()
            for i in range(n):
                rows = fb.critic_rows(obs3, act3 if has_act else None, i, form)
                assert rows.shape == (b, width)
                assert (critic(rows, None)[0] - fb.critic_plain(critic, rows)[0]).abs().max() < 1e-12
        # COMA: the action columns are the last n a of fc1.weight
        critic = fb.make_critic(in_features=(n + 1) * o + n + n * a).double()
        z1 = th.randn(b * n, 64, generator=g).double()
        sampled = act3.unsqueeze(0) + th.randn(4, b, n, a, generator=g).double()
        base, qs, q = coma_baseline(critic, z1, act3, sampled, want_q=True, want_values=True, fused=False)
        pb, pqs, pq, pres = fb.coma_baseline_plain(critic, z1, act3, sampled)
        assert (base - pb).abs().max() < 1e-12 and (qs - pqs).abs().max() < 1e-12 and (q - pq).abs().max() < 1e-12
        assert [tuple(p.shape) for p in pres] == [(4 * b * n, 64)] * 2 + [(b * n, 64)] * 2
    # SQDDPG: values and the own-action gradient of the learner's materialising form
    m = SQDDPG(golden_args("sqddpg3")._replace(sample_size=4)).double()
    with th.no_grad():
        for p in m.value_dicts.parameters():
            p.copy_(0.2 * th.randn_like(p))
    obs = th.randn(b, 3, m.obs_dim, generator=g).double()
    act = th.rand(b, 3, m.act_dim, generator=g).double()
    pos = th.argsort(th.rand(b * 4, 3, generator=g), dim=1).argsort(dim=1)
    up = th.randn(b, 4, 3, generator=g).double()
    a1, a2 = act.clone().requires_grad_(True), act.clone().requires_grad_(True)
    v = m.marginal_contribution_torch(obs, a1, pos).view(b, 4, 3)
    phi, q, pre1, pre2 = fb.sqddpg_plain(m.value_dicts[0], obs, a2, pos, 4)
    assert (v - q).abs().max() < 1e-12 and (phi - v.mean(1)).abs().max() < 1e-12 and pre1.shape == (b * 4 * 3, 64)
    (g1,), (g2,) = th.autograd.grad((v * up).sum(), [a1]), th.autograd.grad((q * up).sum(), [a2])
    assert (g1 - g2).abs().max() < 1e-12 and g1.abs().max() > 0


def test_constant_family_makes_every_rows_layernorm_inputs_equal():
    g = th.Generator().manual_seed(5)
    fam = fb.families(35, 5, 30, g, kind="mlp")["constant"]
    agent = fb.apply_params(fb.make_mlp_agent(30, 5, 4), fam)
    z = agent.fc1(fb.with_ids(fam.inputs[0], 5))
    assert th.equal(z, th.full_like(z, fb.CONSTANT_BIAS))
    # ... and the running sum of 64 such values in fp32 is not 64 times the value: what the family is for
    run = th.zeros(())
    for _ in range(64):
        run = run + th.tensor(fb.CONSTANT_BIAS)
    assert float(run) != float(th.tensor(fb.CONSTANT_BIAS) * 64)
    fam = fb.families(35, 5, 30, g)["constant"]                                # the RNN actor's
    agent = fb.apply_params(fb.make_agent(30, 5, 4), fam)
    z = agent.fc1(fb.with_ids(fam.inputs[0], 5))
    assert th.equal(z, th.full_like(z, fb.CONSTANT_BIAS))


@pytest.mark.parametrize("name,rejected", [("plain", False), ("offset", False), ("constant", True)])
def test_budget_rejects_a_running_sum_layernorm_on_constant_rows(name, rejected):
    """The third wrong evaluation: LayerNorm's statistics accumulated one unit after the other in fp32 in the order of the
    tile scheme's lanes (fb.layer_norm_running_sum).  On plain and offset rows it is one more correct fp32 evaluation; on rows
    of 64 equal inputs its mean is off by an ulp or two, rstd = eps^-1/2 multiplies that, and the budget must say so."""
    n, o, a, rows = 5, 144, 4, 320
    g = th.Generator().manual_seed(3)
    fam = fb.families(rows, n, o, g, kind="mlp")[name]
    agent = fb.apply_params(fb.make_mlp_agent(o, n, a), fam)
    a64 = fb.ref64(agent)
    obs = fam.inputs[0]
    with th.no_grad():
        good = fb.mlp_actor_plain(agent, obs, n)[:2]
        mutant = fb.mlp_actor_plain(agent, obs, n, running_sum=True)[:2]
        ref = fb.mlp_actor_plain(a64, obs.double(), n)[:2]
        # the helper is LayerNorm: in fp64 the two agree
        assert (fb.mlp_actor_plain(a64, obs.double(), n, running_sum=True)[0] - ref[0]).abs().max() < 1e-9
    for k, nm in enumerate(("means", "h")):
        if rejected:
            with pytest.raises(AssertionError):
                fb.within_budget(mutant[k], good[k], ref[k], name=f"mutant running-sum {name} {nm}")
        else:
            fb.within_budget(mutant[k], good[k], ref[k], name=f"running-sum {name} {nm}")


def _share_line(tag, share):
    print(f"tie share {tag}: {share:.4%}")
    assert share <= fb.TIE_CAP, tag


def test_tie_shares_of_the_mlp_actor_cases():
    from . import test_actor_mlp_fp64_gpu as T
    for kind in T.KINDS:
        for family in T.FAMILIES:
            for shape in T.TRAINING:
                agents, _, obs, up = T.case_inputs(kind, *shape, family, "cpu")
                a64 = fb.ref64(agents)
                _share_line(f"actor_mlp {kind} {family} {shape}", fb.clear_ties(lambda o: T.plain(a64, o, th.float64)[2:], (obs,), [up]))


@pytest.mark.parametrize("form", ["maddpg", "ippo"])
def test_tie_shares_of_the_unshared_critic_cases(form):
    from . import test_critic_unshared_fp64_gpu as T
    assert T.FORMS == ("maddpg", "ippo")
    for family in T.FAMILIES:
        for shape in T.SHAPES:
            critics, _, obs, act, up = T.case_inputs(form, *shape, family, "cpu")
            c64 = fb.ref64(critics)
            _share_line(f"critic_unshared {form} {family} {shape}",
                        fb.clear_ties(lambda o, a: T.plain(c64, o, a, form, th.float64)[1:], (obs, act), [up]))


@pytest.mark.parametrize("ns", [1, 10])
@pytest.mark.parametrize("family", ["plain", "reset", "offset", "constant", "constant-act", "dead"])
def test_tie_shares_of_the_sqddpg_cases(family, ns):
    from . import test_sqddpg_fp64_gpu as T
    assert family in T.FAMILIES and set(T.FAMILIES) == {"plain", "reset", "offset", "constant", "constant-act", "dead"}
    assert ns in T.SAMPLE_SIZES and len(T.SAMPLE_SIZES) == 2
    for b, n in T.SHAPES:
        m, obs, act, pos, w, attempt = T.case_inputs(b, n, ns, family, "cpu")
        share, keep = T.clear_tied(fb.ref64(m.value_dicts[0]), obs, act, pos, ns, w)
        _share_line(f"sqddpg {family} {b}x{n} ns={ns} (attempt {attempt})", share)
        tied = T.tied(fb.ref64(m.value_dicts[0]), obs, act, pos, ns)
        assert th.equal(w == 0, tied) and th.equal(keep == 0, tied.any(1))


@pytest.mark.parametrize("b,n,obs_dim,act", [(13, 5, 144, 4), (417, 5, 144, 4), (1025, 2, 30, 2)])
def test_tie_shares_of_the_unshared_rnn_actor_families(b, n, obs_dim, act):
    """tests/test_unshared_fp64_gpu.py's per-agent modules (seeds 10 + i) at its shapes: in the constant and dead families every
    row of an agent has the same LayerNorm output, so one ln_b entry within 1e-5 of zero would clear all of them — none is.
    (The inputs are this generator's, as in the tests above: those of the GPU test come from the device's.)"""
    from . import test_unshared_fp64_gpu as T
    assert (b, n, obs_dim, act) in T.SHAPES and len(T.SHAPES) == 3
    rows = b * n
    for family in T.FAMILIES:
        g = th.Generator().manual_seed(rows + act)
        fam = fb.families(rows, n, obs_dim, g)[family]
        agents = fb.apply_params([fb.make_agent(obs_dim, n, act, seed=10 + i) for i in range(n)], fam)
        a64 = fb.ref64(agents)
        obs, hid = fam.inputs[0].view(b, n, obs_dim), fam.inputs[1].view(b, n, 64)
        up = [th.randn(rows, act, generator=g) / rows]
        _share_line(f"actor_unshared {family} {b}x{n}x{obs_dim}x{act}",
                    fb.clear_ties(lambda o_, h_: [T._per_agent(a64, o_, h_, th.float64)[2]], (obs, hid), up))


def test_row_sum_rounding_is_what_a_running_fp32_sum_does_and_still_rejects_1e_5():
    """fb.row_sum_rounding, the floor of the vector-sum gradients in tests/test_sqddpg_fp64_gpu.py and
    tests/test_critic_unshared_fp64_gpu.py: 2 000 sums of 257 cancelling addends, accumulated in fp32 one after the other — the
    order the figure is derived for — with zero-mean addends and with a drift of half their spread.  Their errors have 0.74 of its sigma (the figure takes a rounding to be within 2^-24 of
    the value; half an ulp is between 2^-25 and 2^-24 of it, root mean square 0.74 * 2^-24 over a binade), 3 sigma holds for
    all but a percent of them, a pairwise sum stays inside it, and the budget with the floor still rejects a gradient off by 1e-5 of itself and a
    sum that leaves one row out."""
    g = th.Generator().manual_seed(11)
    n, m = 257, 2000
    for drift in (0.0, 0.5):
        addends = (th.randn(n, m, generator=g) + drift) / n
        ref = addends.double().sum(0)
        run = th.zeros(m)
        for k in range(n):
            run = run + addends[k]
        floor = fb.row_sum_rounding(addends)
        err = (run.double() - ref).abs()
        sigma = floor / 3.0
        ratio = float((err.square().mean() / sigma.square().mean()).sqrt())
        print(f"running sum, drift {drift}: rms error / sigma = {ratio:.3f}, beyond 3 sigma {float((err > floor).double().mean()):.4%}")
        assert 0.6 <= ratio <= 0.9 and float((err > floor).double().mean()) <= 0.01
    addends = th.randn(n, m, generator=g) / n
    ref = addends.double().sum(0)
    run = th.zeros(m)
    for k in range(n):
        run = run + addends[k]
    floor = fb.row_sum_rounding(addends)
    pairwise = addends.clone()
    pad = th.zeros(512 - n, m)
    pairwise = th.cat((pairwise, pad), 0)
    while pairwise.shape[0] > 1:
        pairwise = pairwise[0::2] + pairwise[1::2]
    assert bool(((pairwise[0].double() - ref).abs() <= floor).all())
    # the budget with the floor: the running sum passes with a tree sum as the yardstick; the two wrong sums do not
    tree = addends.sum(0)
    ulps = fb.floor_ulps(floor, ref)
    print(f"floor: {ulps:.1f} ulps of the gradients' scale")
    assert ulps < 100.0
    fb.within_budget(run, tree, ref, floor_ulps=ulps, name="running fp32 sum of 257 rows")
    with pytest.raises(AssertionError):
        fb.within_budget(run * (1.0 + 1e-5), tree, ref, floor_ulps=ulps, name="mutant running sum (1 + 1e-5)")
    with pytest.raises(AssertionError):
        fb.within_budget(run - addends[-1], tree, ref, floor_ulps=ulps, name="mutant running sum without its last row")
    assert fb.floor_ulps(None, ref) == fb.FLOOR_ULPS


# ---------------------------------------------------------------------------------------------------------------------------
# the QMIX mixer's composition, families and cases (tests/test_qmix_fp64_gpu.py)

@pytest.mark.parametrize("n", [1, 3, 8])
def test_qmix_plain_is_the_mixers_forward(n):
    g = th.Generator().manual_seed(n)
    m = fb.make_mixer(n, 16, seed=n, zero_rows=(n == 3)).double()
    q, x = th.randn(35, n, generator=g).double(), 0.3 * th.randn(35, n * 16, generator=g).double()
    with th.no_grad():
        y, pre = fb.qmix_plain(m, q, x)
        assert y.shape == (35,) and (y - m.forward_torch(q, x).view(-1)).abs().max() < 1e-12
        assert [tuple(p.shape) for p in pre] == [(35, 64)] * 3 + [(35, 64 * n), (35, 64)]
        assert th.equal(pre[0], m.hyper_w_1[0](x)) and th.equal(pre[3], m.hyper_w_1(x)) and th.equal(pre[4], m.hyper_w_final(x))
        # the wrong evaluations are wrong in the backward alone, but for the dropped agent
        for wrong in ("abs_grad_one_at_zero", "elu_slope_one"):
            assert th.equal(fb.qmix_plain(m, q, x, wrong=wrong)[0], y)


def test_qmix_families_are_what_they_say():
    B, n, S = 64, 3, 48
    fams = fb.qmix_families(B, n, S, th.Generator().manual_seed(0))
    assert tuple(sorted(fams)) == tuple(sorted(fb.QMIX_FAMILIES))
    q, x, w = fams["plain"].inputs
    assert not fams["reset"].inputs[1].any() and th.equal(fams["reset"].inputs[0], q)
    assert (fams["elu_neg"].inputs[0] <= 0).all() and (fams["elu_deep"].inputs[0] <= -300).all()
    assert th.equal(fams["big_q"].inputs[0], 100.0 * q)
    mq, mx, _ = fams["mixed"].inputs
    for j, name in enumerate(fb.QMIX_MIXED_OF):
        rows = fams["mixed"].groups == j
        assert rows[:32].any() and th.equal(mq[rows], fams[name].inputs[0][rows]) and th.equal(mx[rows], fams[name].inputs[1][rows])
    m64 = fb.ref64(fb.apply_params(fb.make_mixer(n, 16), fams["dead"]))
    with th.no_grad():
        y, pre = fb.qmix_plain(m64, q.double(), x.double())
        assert all((p < 0).all() for p in pre[:3])                                     # every hidden unit off
        assert th.equal(pre[3], m64.hyper_w_1[2].bias.expand(B, -1))                   # w1 = |hyper_w_1.2.bias|
        taps = {}
        fb.qmix_plain(fb.ref64(fb.make_mixer(n, 16)), fams["elu_deep"].inputs[0].double(), x.double(), taps=taps)
        assert taps["b1"].shape == (B, 64) and taps["v"].shape == (B, 1)
    mz = fb.make_mixer(n, 16, zero_rows=True)
    with th.no_grad():
        pre = fb.qmix_plain(mz, q, x)[1]
        assert not pre[3][:, ::7].any() and not pre[4][:, ::5].any() and pre[3][:, 1].all()


@pytest.mark.parametrize("family", fb.QMIX_FAMILIES)
def test_tie_shares_of_the_qmix_cases_and_the_yardsticks_own_budget(family):
    from . import test_qmix_fp64_gpu as T
    assert family in T.FAMILIES and len(T.FAMILIES) == 8 and len(T.SHAPES) == 6
    for B, n, obs in T.SHAPES:
        m, q, x, w, share, attempt = T.case_inputs(B, n, obs, family, "cpu")
        m64 = fb.ref64(m)
        _share_line(f"qmix {family} {B}x{n}x{obs} (attempt {attempt})", share)
        with th.no_grad():
            tied = fb.tie_rows(fb.qmix_plain(m64, q.double(), x.double())[1])
        assert th.equal(w == 0, tied) and float(tied.double().mean()) == share
        t32, r64 = fb.qmix_run(m, q, x, w, th.float32), fb.qmix_run(m64, q, x, w, th.float64)
        fb.within_budget(t32[0], t32[0], r64[0], name=f"cpu-yardstick qmix {family} {B}x{n}x{obs} q_tot")
        fb.within_budget(t32[1], t32[1], r64[1], name=f"cpu-yardstick qmix {family} {B}x{n}x{obs} d_agent_qs")
        assert set(r64[3]) == set(fb.QMIX_BIAS_ADDENDS) and all(r64[3][k].shape == r64[2][k].shape for k in r64[3])
    for B, n, obs in T.STRUCTURE:
        assert (B, n, obs) in T.SHAPES


# the tensors a wrong evaluation must be rejected on, and the least number of parameter gradients among the rejected
QMIX_REJECTED_ON = {"abs_grad_one_at_zero": (("hyper_w_1.2.weight", "hyper_w_1.2.bias"), 2),
                    "drop_last_agent": (("q_tot", "agent_qs"), 7), "elu_slope_one": (("agent_qs",), 4)}


@pytest.mark.parametrize("B,n,obs", [(33, 8, 16), (129, 5, 144), (31, 3, 16)])
@pytest.mark.parametrize("family", ["plain", "reset", "elu_neg"])
@pytest.mark.parametrize("wrong", fb.QMIX_WRONG)
def test_budget_rejects_three_wrong_evaluations_of_the_mixer(wrong, family, B, n, obs):
    """At three of tests/test_qmix_fp64_gpu.py's shapes, with zero_rows on (what the first wrong evaluation needs; the other
    two do not mind): the right fp32 evaluation is accepted on every tensor, each wrong one is rejected on the tensors named in
    QMIX_REJECTED_ON and on at least the number of parameter gradients given there."""
    g = th.Generator().manual_seed(1000 * B + 10 * obs + n)
    q, x, w = fb.qmix_families(B, n, n * obs, g)[family].inputs
    m = fb.make_mixer(n, obs, seed=1, zero_rows=True)
    m64 = fb.ref64(m)
    fb.qmix_clear_ties(m64, x, w)
    good, ref = fb.qmix_run(m, q, x, w, th.float32), fb.qmix_run(m64, q, x, w, th.float64)
    bad = fb.qmix_run(m, q, x, w, th.float32, wrong=wrong)

    def tensors(run):
        return dict(q_tot=run[0], agent_qs=run[1], **run[2])

    rejected = []
    for name, r in tensors(ref).items():
        fb.within_budget(tensors(good)[name], tensors(good)[name], r, name=f"right evaluation {family} {B}x{n}x{obs} {name}")
        try:
            fb.within_budget(tensors(bad)[name], tensors(good)[name], r, name=f"mutant {wrong} {family} {B}x{n}x{obs} {name}")
        except AssertionError:
            rejected.append(name)
    print(f"{wrong} {family} {B}x{n}x{obs}: rejected on {rejected}")
    named, least = QMIX_REJECTED_ON[wrong]
    assert set(named) <= set(rejected) and len(set(rejected) - {"q_tot", "agent_qs"}) >= least, rejected


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/ppo.hip, csrc/gauss.hip and the stand-alone csrc/tdloss.hip: the compositions, families and cases of
# tests/test_ppo_fp64_gpu.py, test_gauss_fp64_gpu.py and test_tdloss_fp64_gpu.py

def _rejected(mutant, good, ref, name):
    with pytest.raises(AssertionError):
        fb.within_budget(mutant, good, ref, name=name)


def test_ppo_gauss_and_td_compositions_are_the_existing_functions():
    from safe_marl_amd import nets
    g = th.Generator().manual_seed(0)
    # GAE: the wrapper is nets.ppo_gae, the literal per-chain loop is nets.ppo_gae_torch on whole steps
    fam = fb.gae_families(320, 5, 4, g)["plain"]
    x = [t.double() for t in fam.inputs]
    out = fb.gae_plain(*x, fb.GAMMA, fb.LAM, 4, fb.bn_module(5, th.float64, seed=1), fb.bn_module(5, th.float64, seed=2))
    rbn, abn = fb.bn_module(5, th.float64, seed=1), fb.bn_module(5, th.float64, seed=2)
    with th.no_grad():
        rn = rbn(x[0])
        adv = nets.ppo_gae_torch(rn, *x[1:], fb.GAMMA, fb.LAM, 4)
        advn = abn(adv)
    for got, want in ((out["reward_norm"], rn), (out["advantages"], adv), (out["advantages_norm"], advn),
                      (out["reward_bn.running_var"], rbn.running_var), (out["adv_bn.running_mean"], abn.running_mean),
                      (fb.gae_chain_loop(rn, *x[1:], fb.GAMMA, fb.LAM, 4), adv)):
        assert (got - want).abs().max() < 1e-12
    assert int(out["adv_bn.num_batches_tracked"]) == 1
    # ragged chains: every chain is ppo_gae_torch on its own rows
    rows, stride = 29, 8
    fam = fb.gae_families(rows, 3, stride, g)["plain"]
    x = [t.double() for t in fam.inputs]
    loop = fb.gae_chain_loop(*x, fb.GAMMA, fb.LAM, stride)
    for e in range(stride):
        own = nets.ppo_gae_torch(*[t[e::stride] for t in x], fb.GAMMA, fb.LAM, 1)
        assert (loop[e::stride] - own).abs().max() < 1e-12
    # the losses: the wrong evaluations are wrong in one gradient alone, so their values pin the hand-written forms
    fam = fb.policy_families(33, 3, 4, g)["plain"]
    good, bad = fb.policy_loss_plain(fam.inputs, 0.2, th.float64), fb.policy_loss_plain(fam.inputs, 0.2, th.float64, wrong="no_minus_one")
    m = fam.inputs[0].double().requires_grad_(True)
    loss, ratio = nets.ppo_policy_loss_torch(m, fam.inputs[1].double(), *[t.double() for t in fam.inputs[2:]], 0.2)
    assert th.equal(good["loss"], loss.detach()) and th.equal(good["ratio"], ratio.detach())
    for k in ("loss", "ratio", "d_means"):
        assert (good[k] - bad[k]).abs().max() < 1e-12
    assert (good["d_log_stds"] - bad["d_log_stds"]).abs().max() > 1e-4
    fixed = fb.policy_loss_plain(fam.inputs, 0.2, th.float64, fixed=True)
    assert set(fixed) == {"loss", "ratio", "d_means"}
    fam = fb.value_families(33, 3, g)["plain"]
    good, bad = fb.value_loss_plain(fam.inputs, 0.5, fb.GAMMA, 2.0, th.float64), fb.value_loss_plain(fam.inputs, 0.5, fb.GAMMA, 2.0, th.float64, wrong="clamp_open")
    loss, ret = nets.ppo_value_loss_torch(*[t.double() for t in fam.inputs], fb.GAMMA, 0.5, 2.0)
    assert th.equal(good["loss"], loss) and th.equal(good["returns"], ret)
    assert (good["loss"] - bad["loss"]).abs() < 1e-12 and (good["returns"] - bad["returns"]).abs().max() < 1e-12
    # the head: log_std is nets.gauss_log_std_torch, for the shared head and for every agent's own on its rows
    fam = fb.gauss_families(33, 4, g)["plain"]
    h, w, b = (t.double() for t in fam.inputs[:3])
    out = fb.gauss_head_plain(fam.inputs, -5.0, 2.0, th.float64)
    assert (out["log_std"] - nets.gauss_log_std_torch(h, w, b, -5.0, 2.0)).abs().max() < 1e-12
    assert (fb.gauss_head_plain(fam.inputs, -5.0, 2.0, th.float64, wrong="one_minus_t")["log_std"] - out["log_std"]).abs().max() < 1e-12
    fam = fb.gauss_families(33 * 3, 4, g, n=3)["plain"]
    h, w, b = (t.double() for t in fam.inputs[:3])
    out = fb.gauss_head_plain(fam.inputs, 0.0, 0.5, th.float64)
    for i in range(3):
        assert (out["log_std"][i::3] - nets.gauss_log_std_torch(h[i::3], w[i], b[i], 0.0, 0.5)).abs().max() < 1e-12
    assert out["d_w"].shape == (3, 4, 64) and out["d_b"].shape == (3, 4)
    # the TD loss through a module is td_loss_plain on batch statistics
    fam = fb.td_families(33, 5, g)["plain"]
    bn = fb.bn_module(5, th.float64, seed=3)
    q, nq, r, d = (t.double() for t in fam.inputs)
    want = fb.td_loss_plain(q, nq, r, d, fb.GAMMA, bn)
    out = fb.td_run(fam.inputs, fb.GAMMA, bn, th.float64)
    assert (out["loss"] - want).abs() < 1e-12 and int(out["num_batches_tracked"]) == 1


def test_gae_families_are_what_they_say():
    from . import test_ppo_fp64_gpu as T
    assert set(fb.gae_families(24, 3, 8, th.Generator().manual_seed(0))) == set(fb.GAE_FAMILIES)
    for rows, n, stride in T.GAE_SHAPES[:5] + T.GAE_RAGGED:
        fams = {name: T.gae_case(rows, n, stride, name) for name in fb.GAE_FAMILIES}
        r, v, nv, done, last = fams["plain"].inputs
        combos = {(int(d), int(l)) for d, l in zip(done.tolist(), last.tolist())}
        assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)} or rows < 100, combos     # done = 1 on rows that are no last step
        assert fams["all_terminal"].inputs[3].all() and fams["all_terminal"].inputs[4].all()
        assert not fams["open_sum"].inputs[4].any() and fams["open_sum"].params == {"gamma": 1.0, "lam": 1.0}
        assert fams["open_sum"].inputs[3].any() or rows < 100
        assert fams["gamma0"].params["gamma"] == 0.0
        after, steps_of = fb.steps_from_end(rows, stride)
        d, l = fams["tile_edges"].inputs[3:]
        want = (after % 64 == 0) | (after % 64 == 63) | (after == steps_of - 1)
        assert th.equal(d, l) and th.equal(d.bool(), want)
        assert d[after == 0].all() and d[after == 63].all() and d[(after > 0) & (after < 63) & (after < steps_of - 1)].sum() == 0
        rf = fams["failure"].inputs[0]
        assert (rf[:, 0] == fb.FAILURE_REWARD).all() and float(rf[:, 0].double().var(unbiased=False)) == 0.0
        if rows > 100:
            assert 0.8 * fb.FAILURE_SPREAD < float(rf[:, 1].double().std()) < 1.2 * fb.FAILURE_SPREAD
        assert th.equal(rf[:, 2:], r[:, 2:])
        g = fams["mixed"].groups
        for j, name in enumerate(fb.GAE_MIXED_OF):
            sel = g == j
            assert th.equal(fams["mixed"].inputs[3][sel], fams[name].inputs[3][sel])
            assert th.equal(fams["mixed"].inputs[4][sel], fams[name].inputs[4][sel])
            assert th.equal(sel, (th.arange(rows) % stride) % len(fb.GAE_MIXED_OF) == j)       # chain by chain
    # all_terminal: A = delta = r - V, no carry and no bootstrap; open_sum: the suffix sums of delta over the whole chain
    fam = T.gae_case(320, 5, 1, "all_terminal")
    x = [t.double() for t in fam.inputs]
    assert th.equal(fb.gae_plain(*x, fb.GAMMA, fb.LAM, 1)["advantages"], x[0] - x[1])
    fam = T.gae_case(320, 5, 1, "open_sum")
    x = [t.double() for t in fam.inputs]
    delta = x[0] + x[2] - x[1]
    assert (fb.gae_plain(*x, 1.0, 1.0, 1)["advantages"] - delta.flip(0).cumsum(0).flip(0)).abs().max() < 1e-11


def test_policy_value_and_head_families_are_what_they_say():
    rows, n, a = 257, 5, 4
    for per_row in (True, False):
        for rng in fb.LOG_STD_RANGES:
            fams = fb.policy_families(rows, n, a, th.Generator().manual_seed(1), per_row=per_row, log_std_range=rng)
            assert set(fams) == set(fb.POLICY_FAMILIES)
            for name, fam in fams.items():
                means, ls, act, old, adv = fam.inputs
                assert all(th.equal(act[:, i], act[:, 0]) for i in range(n)), name            # one action for every agent
                if not per_row and name != "mixed":
                    assert (ls == ls[0, 0, 0]).all(), name
            means, ls, act, old, adv = fams["on_mean"].inputs
            mu = means[:, 0]
            for i in range(1, n):
                mu = mu + means[:, i]                                                   # fp32, agent order
            assert th.equal(act[:, 0], mu) and th.equal(mu.double(), means.double().sum(1))   # d is exactly zero in fp32
            out = fb.policy_loss_plain(fams["on_mean"].inputs, 0.2, th.float32, fixed=not per_row)
            assert not out["d_means"].any()
            assert not fams["zero_adv"].inputs[4].any()
            out = fb.policy_loss_plain(fams["clipped_out"].inputs, 0.2, th.float64, fixed=not per_row)
            adv = fams["clipped_out"].inputs[4].double()
            assert adv.all() and ((out["ratio"] > 1.2) == (adv > 0)).all() and ((out["ratio"] < 0.8) == (adv < 0)).all()
            assert not out["d_means"].any()                                            # no ratio inside the range, no gradient
            for name, end in zip(("ends_min", "ends_max"), rng):
                assert (fams[name].inputs[1] == end).all()
                r = fb.policy_loss_plain(fams[name].inputs, 0.2, th.float64, fixed=not per_row)["ratio"]
                assert 0.5 < float(r.min()) and float(r.max()) < 2.0                    # ratios of order one ...
            lp = fb._log_density64(*fams["ends_min"].inputs[:3])
            assert rng[0] == 0.0 or float(lp.abs().min()) > 50.0                        # ... while log p is of order 100
            g = fams["mixed"].groups
            for j, name in enumerate(fb.POLICY_MIXED_OF):
                assert all(th.equal(t[g == j], s[g == j]) for t, s in zip(fams["mixed"].inputs, fams[name].inputs))
    wide = fb.policy_families(100000, 5, 4, th.Generator().manual_seed(77), log_std_range=fb.LOG_STD_RANGES[0])["wide"]
    assert float(fb.policy_loss_plain(wide.inputs, 0.2, th.float64)["ratio"].max()) > 10.0    # the large-ratio regime
    # the value loss
    fams = fb.value_families(rows, n, th.Generator().manual_seed(2))
    assert set(fams) == set(fb.VALUE_FAMILIES)
    v, old, nv, rn, done = fams["plain"].inputs
    assert (v[0::16] - old[0::16] == 0.5).all() and (v[1::16] - old[1::16] == -0.5).all()
    assert fams["eps0"].params["eps_clip"] == 0.0 and th.equal(fams["eps0"].inputs[0][3::16], old[3::16])
    assert fams["all_done"].inputs[4].all()
    # the head
    for n_agents in (None, 3):
        rows_h = 129 if n_agents is None else 43 * 3
        fams = fb.gauss_families(rows_h, 8, th.Generator().manual_seed(3), n=n_agents)
        assert set(fams) == set(fb.GAUSS_FAMILIES)
        assert not fams["reset"].inputs[0].any()
        out = fb.gauss_head_plain(fams["reset"].inputs, -5.0, 2.0, th.float64)
        b = fams["reset"].inputs[2].double()
        assert th.equal(out["t"], th.tanh(b.expand(rows_h, 8) if n_agents is None else b.repeat(43, 1)))   # u = b
        assert (fams["saturated"].inputs[0].abs() == 40.0).all()
        for lo, hi in fb.LOG_STD_RANGES:
            out = fb.gauss_head_plain(fams["saturated"].inputs, lo, hi, th.float64)
            assert (out["t"].abs() == 1).all() and ((out["log_std"] == lo) | (out["log_std"] == hi)).all()
            assert not out["d_u"].any() and not out["d_h"].any() and not out["d_w"].any()
        lo, hi = fams["flat"].params["range"]
        out = fb.gauss_head_plain(fams["flat"].inputs, lo, hi, th.float64)
        assert lo == hi and (out["log_std"] == lo).all() and not out["d_h"].any() and not out["d_b"].any()
        for low, high in ((0.0, 1.0), (-1.0, 1.0)):
            out = fb.gauss_head_plain(fams["wide_noise"].inputs, -5.0, 2.0, th.float32, low, high)
            clamped = out["action"].clamp(low, high)
            assert (clamped == low).any() and (clamped == high).any()                   # env_action on both clamp ends
            assert (out["env_action"] == out["env_action"].min()).sum() > 1 and (out["env_action"] == high).any()
        g = fams["mixed"].groups
        assert set(g[:32].tolist()) == {0, 1, 2} or n_agents is not None                # one 32-row tile holds each kind
        assert not fams["mixed"].inputs[0][g == 1].any() and th.equal(fams["mixed"].inputs[0][g == 2], fams["saturated"].inputs[0][g == 2])
        out = fb.gauss_head_plain(fams["mixed"].inputs, -5.0, 2.0, th.float64)
        assert (out["t"][g == 2].abs() == 1).all() and (out["t"][g == 0].abs() < 1).all()
    fams = fb.td_families(4099, 5, th.Generator().manual_seed(4))
    assert set(fams) == set(fb.TD_FAMILIES) and (fams["failure"].inputs[2][:, 0] == fb.FAILURE_REWARD).all()


def test_kink_shares_of_the_ppo_loss_cases():
    """The very cases of tests/test_ppo_fp64_gpu.py: the share of policy elements whose ratio is within 1e-5 of a clip end, and
    of value elements left out of the d_values comparison, is at most fb.TIE_CAP — and the cleared advantages are zero."""
    from . import test_ppo_fp64_gpu as T
    assert len(T.POLICY_SHAPES) == 6 and len(T.POLICY_CASES) == len(fb.POLICY_FAMILIES) + 2
    worst = 0.0
    for per_row in (False, True):
        for rows, n, a in T.POLICY_SHAPES:
            for family, which in T.POLICY_CASES:
                fam, share = T.policy_case(rows, n, a, family, per_row, which)
                assert share <= fb.TIE_CAP, (per_row, rows, n, a, family, which, share)
                assert fb.policy_clear_kinks(fam.inputs, fam.params["eps_clip"]) == 0.0       # cleared: none is left
                worst = max(worst, share)
    print(f"kink share, policy cases: at most {worst:.4%}")
    worst = 0.0
    for rows, n in T.VALUE_SHAPES:
        for family in fb.VALUE_FAMILIES:
            fam, keep = T.value_case(rows, n, family)
            share = 1.0 - float(keep.double().mean())
            assert share <= fb.TIE_CAP, (rows, n, family, share)
            for k in range(4):
                assert keep[k::16].all()                                               # the constructed rows are compared
            worst = max(worst, share)
    print(f"share left out of d_values, value cases: at most {worst:.4%}")


@pytest.mark.parametrize("rows,n,stride", [(514, 3, 2), (320, 5, 1), (1000, 5, 1)])
@pytest.mark.parametrize("wrong", ["mask_everywhere", "drop_carry_64"])
def test_budget_rejects_two_wrong_gae_evaluations(wrong, rows, n, stride):
    """m = 1 - done on every row (what every GPU test accepted while done was drawn inside last_step), and a scan that drops
    its carry between 64-step tiles, at the wave kernel's shapes of tests/test_ppo_fp64_gpu.py, with and without the modules."""
    from . import test_ppo_fp64_gpu as T
    assert (rows, n, stride) in T.GAE_SHAPES
    families = ("plain", "mixed", "failure") if wrong == "mask_everywhere" else ("plain", "open_sum", "gamma0")
    for family in families:
        fam = T.gae_case(rows, n, stride, family)
        gamma, lam = fam.params["gamma"], fam.params["lam"]
        for bn in (True, False):
            mods = lambda dtype: (fb.bn_module(n, dtype, seed=1), fb.bn_module(n, dtype, seed=2)) if bn else (None, None)
            ref = fb.gae_plain(*[x.double() for x in fam.inputs], gamma, lam, stride, *mods(th.float64))
            good = fb.gae_plain(*fam.inputs, gamma, lam, stride, *mods(th.float32))
            bad = fb.gae_plain(*fam.inputs, gamma, lam, stride, *mods(th.float32), wrong=wrong)
            tag = f"{wrong} {family} {rows}x{n}/{stride} bn={int(bn)}"
            fb.within_budget(good["advantages"], good["advantages"], ref["advantages"], name=f"right evaluation {tag} advantages")
            if wrong == "drop_carry_64" and family == "gamma0":
                # gamma = 0: there is no carry to drop — the family that cannot see this error, and must not
                fb.within_budget(bad["advantages"], good["advantages"], ref["advantages"], name=f"mutant {tag} advantages (harmless)")
                continue
            _rejected(bad["advantages"], good["advantages"], ref["advantages"], f"mutant {tag} advantages")
            _rejected(bad["advantages_norm"], good["advantages_norm"], ref["advantages_norm"], f"mutant {tag} advantages_norm")
            if bn:
                _rejected(bad["adv_bn.running_mean"], good["adv_bn.running_mean"], ref["adv_bn.running_mean"], f"mutant {tag} adv_bn.running_mean")


@pytest.mark.parametrize("rows,n,stride", [(2, 5, 1), (24, 3, 8), (320, 5, 1)])
def test_budget_rejects_a_running_variance_from_the_biased_batch_variance(rows, n, stride):
    """nn.BatchNorm1d moves running_var by the UNBIASED batch variance: a factor rows / (rows - 1), 2 on the smallest batch.
    (On the advantages at every one of these shapes; on the reward, whose variance of 2.5e-3 sits under a running variance
    of order one, while the factor is at least 1 / 23.)"""
    from . import test_ppo_fp64_gpu as T
    assert (rows, n, stride) in T.GAE_SHAPES
    fam = T.gae_case(rows, n, stride, "plain")
    mods = lambda dtype: (fb.bn_module(n, dtype, seed=1), fb.bn_module(n, dtype, seed=2))
    ref = fb.gae_plain(*[x.double() for x in fam.inputs], fb.GAMMA, fb.LAM, stride, *mods(th.float64))
    good = fb.gae_plain(*fam.inputs, fb.GAMMA, fb.LAM, stride, *mods(th.float32))
    bad = fb.gae_plain(*fam.inputs, fb.GAMMA, fb.LAM, stride, *mods(th.float32), wrong="biased_running_var")
    for key in ("adv_bn", "reward_bn"):
        fb.within_budget(good[key + ".running_var"], good[key + ".running_var"], ref[key + ".running_var"], name=f"right {key}.running_var {rows}")
        assert th.equal(bad[key + ".running_mean"], good[key + ".running_mean"])
        if key == "adv_bn" or rows <= 24:
            _rejected(bad[key + ".running_var"], good[key + ".running_var"], ref[key + ".running_var"], f"mutant biased {key}.running_var {rows}x{n}")


@pytest.mark.parametrize("rows,n,a", [(33, 3, 4), (65, 5, 8), (257, 8, 8), (300, 5, 3)])
def test_budget_rejects_wrong_gradients_of_the_losses_and_the_head(rows, n, a):
    """d log p / d log_std without its - 1 (on plain rows and on rows whose action is on the mean, where the - 1 is all there
    is), clamp's gradient cut at its ends in the value loss, and the head's d_u with 1 - t in place of 1 - t^2 — at shapes of
    the GPU tests."""
    from . import test_gauss_fp64_gpu as G
    from . import test_ppo_fp64_gpu as T
    assert (rows, n, a) in T.POLICY_SHAPES
    for family in ("plain", "on_mean", "mixed"):
        fam, _ = T.policy_case(rows, n, a, family, True, 0)
        ref, good = fb.policy_loss_plain(fam.inputs, 0.2, th.float64), fb.policy_loss_plain(fam.inputs, 0.2, th.float32)
        bad = fb.policy_loss_plain(fam.inputs, 0.2, th.float32, wrong="no_minus_one")
        for name in ("loss", "ratio", "d_means"):
            fb.within_budget(bad[name], good[name], ref[name], name=f"mutant no_minus_one {family} {rows}x{n}x{a} {name} (unchanged)")
        _rejected(bad["d_log_stds"], good["d_log_stds"], ref["d_log_stds"], f"mutant no_minus_one {family} {rows}x{n}x{a} d_log_stds")
    for family in ("plain", "all_done"):
        fam, keep = T.value_case(rows, n, family)
        eps = fam.params["eps_clip"]
        ref, good = fb.value_loss_plain(fam.inputs, eps, fb.GAMMA, T.COEF, th.float64), fb.value_loss_plain(fam.inputs, eps, fb.GAMMA, T.COEF, th.float32)
        bad = fb.value_loss_plain(fam.inputs, eps, fb.GAMMA, T.COEF, th.float32, wrong="clamp_open")
        fb.within_budget(good["d_values"][keep], good["d_values"][keep], ref["d_values"][keep], name=f"right evaluation value {family} d_values")
        _rejected(bad["d_values"][keep], good["d_values"][keep], ref["d_values"][keep], f"mutant clamp_open {family} {rows}x{n} d_values")
    for n_agents, shape in ((None, (G.ROWS[-1], G.ACTS[-1])), (n, (rows * n, a))):
        for family in ("plain", "mixed"):
            fam, ranges = G.head_case(*shape, family, n=n_agents)
            lo, hi = ranges[-1]
            ref, good = fb.gauss_head_plain(fam.inputs, lo, hi, th.float64), fb.gauss_head_plain(fam.inputs, lo, hi, th.float32)
            bad = fb.gauss_head_plain(fam.inputs, lo, hi, th.float32, wrong="one_minus_t")
            fb.within_budget(bad["log_std"], good["log_std"], ref["log_std"], name=f"mutant one_minus_t {family} log_std (unchanged)")
            for name in ("d_h", "d_w", "d_b"):
                _rejected(bad[name], good[name], ref[name], f"mutant one_minus_t {family} {shape} {name}")


def test_the_yardsticks_of_the_ppo_gauss_and_td_cases_pass_their_own_budget():
    """Every form the GPU tests compare a kernel with runs on a sample of their cases, fp32 against fp64, and is finite."""
    from . import test_gauss_fp64_gpu as G
    from . import test_ppo_fp64_gpu as T
    from . import test_tdloss_fp64_gpu as D
    for rows, n, stride in T.GAE_SHAPES[:5] + T.GAE_SHAPES[6:] + T.GAE_RAGGED:
        for family in fb.GAE_FAMILIES:
            fam = T.gae_case(rows, n, stride, family)
            for bn in (True, False):
                ref, t32 = T._gae_forms(fam, n, stride, bn)
                for name, r in ref.items():
                    assert th.isfinite(r).all() and th.isfinite(t32[name]).all(), (rows, family, name)
                    if not name.endswith("num_batches_tracked"):
                        fb.within_budget(t32[name], t32[name], r, name=f"cpu-yardstick gae {family} {rows}x{n}/{stride} {name}")
    for rows in D.ROWS[:3]:
        for n in D.AGENTS:
            for family in fb.TD_FAMILIES:
                fam = D.td_case(rows, n, family)
                bn = lambda dtype: fb.bn_module(n, dtype, seed=3) if rows > 1 else None
                ref, t32 = fb.td_run(fam.inputs, fb.GAMMA, bn(th.float64), th.float64), fb.td_run(fam.inputs, fb.GAMMA, bn(th.float32), th.float32)
                for name, r in ref.items():
                    assert th.isfinite(r).all() and th.isfinite(t32[name]).all(), (rows, n, family, name)
    for b, n, a in G.UNSHARED:
        for family in fb.GAUSS_FAMILIES:
            fam, ranges = G.head_case(b * n, a, family, n=n)
            for lo, hi in ranges:
                ref, t32 = fb.gauss_head_plain(fam.inputs, lo, hi, th.float64), fb.gauss_head_plain(fam.inputs, lo, hi, th.float32)
                assert all(th.isfinite(t).all() for t in ref.values()) and all(th.isfinite(t).all() for t in t32.values())
                assert G._log_std_floor(lo, hi, ref["log_std"]) >= fb.FLOOR_ULPS


@pytest.mark.parametrize("family,shape,per_row", [("plain", (33, 3, 4), True), ("plain", (257, 8, 8), False), ("mixed", (65, 5, 8), True),
                                                  ("ends_max", (300, 5, 3), True), ("ends_min", (65, 5, 8), False)])
def test_policy_loss_rounding_is_what_the_fp32_composition_does_and_still_rejects_a_dropped_row(family, shape, per_row):
    """fb.policy_loss_rounding, the floor a policy loss takes where it misses the plain budget (tests/test_ppo_fp64_gpu.py says
    which): over 60 draws at a GPU shape the fp32 composition's loss is off by 0.4 to 0.9 of its sigma (root mean square) and
    never by more than the 3 sigma of the figure; and the budget with the floor still rejects a loss that leaves one row out."""
    from . import test_ppo_fp64_gpu as T
    assert shape in T.POLICY_SHAPES
    ratios = []
    for seed in range(60):
        fam = fb.policy_families(*shape, th.Generator().manual_seed(seed), per_row=per_row, log_std_range=fb.LOG_STD_RANGES[1])[family]
        fb.policy_clear_kinks(fam.inputs, fb.POLICY_EPS)
        ref = fb.policy_loss_plain(fam.inputs, fb.POLICY_EPS, th.float64, fixed=not per_row)["loss"]
        t32 = fb.policy_loss_plain(fam.inputs, fb.POLICY_EPS, th.float32, fixed=not per_row)["loss"]
        floor = float(fb.policy_loss_rounding(fam.inputs, fb.POLICY_EPS))
        ratios.append(abs(float(t32) - float(ref)) / (floor / 3.0))
    ratios = th.tensor(ratios)
    rms = float(ratios.square().mean().sqrt())
    print(f"policy_loss_rounding {family} {shape}: rms error / sigma = {rms:.2f}, largest {float(ratios.max()):.2f}")
    assert 0.3 <= rms <= 1.0 and float(ratios.max()) <= 3.0
    # the last draw: the right loss passes with the floor, a loss without its last row does not
    extra = floor / (fb.ULP * abs(float(ref)))
    fb.within_budget(t32, t32, ref, floor_ulps=fb.FLOOR_ULPS + extra, name=f"right loss {family} {shape}")
    short = tuple(t[:-1] for t in fam.inputs)
    wrong = fb.policy_loss_plain(short, fb.POLICY_EPS, th.float32, fixed=not per_row)["loss"] * (shape[0] - 1) / shape[0]
    _rejected(wrong, t32, ref, f"mutant loss without its last row {family} {shape}")


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/wgrad.hip and csrc/linear.hip: the products, floors, families and cases of tests/test_wgrad_fp64_gpu.py and
# tests/test_linear_fp64_gpu.py.  The yardstick here is the CPU's fp32 matmul; on the GPU it is the library GEMM.

@pytest.mark.parametrize("k,m,n", [(37, 5, 7), (130, 4, 9)])
def test_product_sum_rounding_is_row_sum_rounding_of_the_materialised_addends(k, m, n):
    g = th.Generator().manual_seed(k)
    dy, x = th.randn(k, m, generator=g), th.randn(k, n, generator=g) + 0.5
    addends = dy.double()[:, :, None] * x.double()[:, None, :]
    want = fb.row_sum_rounding(addends)
    got = fb.product_sum_rounding(dy, x)
    assert got.shape == (m, n) and float(((got - want).abs() / want).max()) <= 1e-12
    # one run of ordered_sum_rounding is the same figure; two runs of exchangeable rows stay of its size
    two = fb.product_sum_rounding(dy, x, split=(k + 1) // 2)
    assert 0.7 <= float(two.square().mean().sqrt() / want.square().mean().sqrt()) <= 1.4
    # flexnet_linear2's floor: the same thing over the input columns
    W = th.randn(64, k + 5, generator=g)
    x1, x2 = th.randn(m, k - 4, generator=g), th.randn(m, 4, generator=g)
    cols = th.cat((W[:, :k - 4], W[:, k + 1:]), 1).double()
    addends = th.cat((x1, x2), 1).double().t()[:, :, None] * cols.t()[:, None, :]
    want = fb.row_sum_rounding(addends)
    got = fb.linear2_sum_rounding(x1, x2, W, 0, k + 1)
    assert got.shape == (m, 64) and float(((got - want).abs() / want).max()) <= 1e-12


def test_wgrad_and_linear2_families_are_what_they_say():
    fams = fb.wgrad_case(130, 4, 64)
    assert tuple(fams) == fb.WGRAD_FAMILIES
    dy, x = fams["constant"].inputs
    assert bool((dy == fb.CONSTANT_BIAS).all()) and bool((x == fb.CONSTANT_X).all())
    dy, x = fams["halves"].inputs
    assert fams["halves"].params["split"] == 65 and bool((x[:65] > 25).all()) and bool((x[65:] < -25).all())
    ref = fb.wgrad_plain(dy.double(), x.double())[0]
    assert float(ref.abs().max()) < 0.1 * 15 * 130                      # the rows cancel: far below the partial sums
    assert not fams["zero_x"].inputs[1].any() and not fams["zero_dy"].inputs[0].any()
    assert th.equal(fams["zero_x"].inputs[0], fams["plain"].inputs[0])
    mx, groups = fams["mixed"].inputs[1], fams["mixed"].groups
    assert not mx[groups == 1].any() and th.equal(mx[groups == 2], 30.0 * fams["plain"].inputs[1][groups == 2])
    assert set(groups[:8].tolist()) == {0, 1, 2} and set(groups[64:72].tolist()) == {0, 1, 2}
    again = fb.wgrad_case(130, 4, 64)
    assert all(th.equal(a, b) for nm in fams for a, b in zip(fams[nm].inputs, again[nm].inputs))
    # every class is reached by its shapes, on both sides of each boundary
    from safe_marl_amd.nets import _wgrad_class
    for cls, shape, _ in fb.wgrad_cases():
        assert _wgrad_class(shape[1], shape[2])[:2] == cls, (cls, shape)
    assert len(fb.WGRAD_SHAPES) == 8 and all(len(v) >= 2 for v in fb.WGRAD_SHAPES.values())
    ms = {s[1] for v in fb.WGRAD_SHAPES.values() for s in v}
    ns = {s[2] for v in fb.WGRAD_SHAPES.values() for s in v}
    assert {32, 33, 64, 65} <= ms and {32, 33, 64, 65, 160, 161} <= ns
    fams = fb.linear2_case(33, 8, 4)
    assert tuple(fams) == fb.LINEAR2_FAMILIES
    bias, x1, x2, W = fams["plain"].inputs
    assert x1.shape == (33, 8) and x2.shape == (33, 4) and W.shape == (64, 17)
    assert bool(W[:, 8:13].isnan().all()) and bool(W[:, :8].isfinite().all()) and bool(W[:, 13:].isfinite().all())
    assert [fb.linear2_ss(*w) for w in fb.LINEAR2_WIDTHS] == [1, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3]
    assert fb.linear2_ss(768, 8) == 4                                   # refused


def _wgrad_cannot_differ(k, m, n, family, wrong, tensor):
    """The cases in which a wrong evaluation of WGRAD_WRONG is the right one (``tensor``: "C" or "colsum")."""
    if family == "zero_dy" or (family == "zero_x" and tensor == "C"):
        return "a zero family"
    if wrong == "colsum_per_chunk":
        return "C is not touched" if tensor == "C" else ("one column chunk" if fb.wgrad_chunks(m, n) == 1 else None)
    if wrong == "drop_slab_tail" and k % 8 == 0:
        return "k is whole 8-row groups"
    if family == "mixed" and tensor == "C":
        dropped = [k - 1] if wrong == "drop_last_row" else list(range(k - k % 8, k))
        if all(r % 3 == 1 for r in dropped):
            return "mixed: the rows left out are zero rows of x"
    return None


# One case in which the budget cannot tell a wrong evaluation that DOES differ: one of 32 777 equal rows is 2^-15 of the sum,
# 512 ulps, and the row-order running sum the budget must admit is itself off by 2 440 ulps there (fb.equal_addend_drift).  The
# plain family at the same shape rejects both row drops.
WGRAD_BELOW_THE_DRIFT = {(fb.WGRAD_CAP_SHAPE, "constant", "drop_last_row"), (fb.WGRAD_CAP_SHAPE, "constant", "drop_slab_tail")}


@pytest.mark.parametrize("cls,shape,names", fb.wgrad_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else None)
def test_wgrad_cases_admit_a_row_order_running_sum_and_reject_the_wrong_evaluations(cls, shape, names):
    """For every (shape, family) of tests/test_wgrad_fp64_gpu.py: dW and the column sum accumulated in fp32 one row after the
    other — the least accurate order a correct kernel may use — are inside the budget with the floors the GPU test takes
    (fb.wgrad_floors), and each of fb.WGRAD_WRONG, evaluated in fp32, is outside it, on dW and on the column sum, unless it
    cannot differ (``_wgrad_cannot_differ``, checked in fp64) or is in WGRAD_BELOW_THE_DRIFT."""
    k, m, n = shape
    fams = fb.wgrad_case(k, m, n)
    dys = th.stack([fams[nm].inputs[0] for nm in names])
    xs = th.stack([fams[nm].inputs[1] for nm in names])
    run_c, run_cs = th.zeros(len(names), m, n), th.zeros(len(names), m)
    for r in range(k):
        run_c = run_c + dys[:, r, :, None] * xs[:, r, None, :]
        run_cs = run_cs + dys[:, r]
    for i, nm in enumerate(names):
        dy, x = fams[nm].inputs
        ref = dict(zip(("C", "colsum"), fb.wgrad_plain(dy.double(), x.double())))
        yard = dict(zip(("C", "colsum"), fb.wgrad_plain(dy, x)))
        floors = dict(zip(("C", "colsum"), fb.wgrad_floors(fams[nm])))
        ulps = {t: fb.floor_ulps(floors[t], ref[t]) for t in ref}
        for t, run in (("C", run_c[i]), ("colsum", run_cs[i])):
            fb.within_budget(run, yard[t], ref[t], floor_ulps=ulps[t], name=f"running sum {k}x{m}x{n} {nm} {t} (floor {ulps[t]:.0f} ulps)")
        if nm in ("zero_x", "zero_dy"):
            assert not ref["C"].any() and ulps["C"] == fb.FLOOR_ULPS
        for wrong in fb.WGRAD_WRONG:
            bad = dict(zip(("C", "colsum"), fb.wgrad_plain(dy, x, wrong=wrong)))
            bad64 = dict(zip(("C", "colsum"), fb.wgrad_plain(dy.double(), x.double(), wrong=wrong)))
            for t in ("C", "colsum"):
                why = _wgrad_cannot_differ(k, m, n, nm, wrong, t)
                if why is not None:
                    # (to fp64 rounding: without a row the fp64 GEMM may block the others differently)
                    assert float((bad64[t] - ref[t]).abs().max()) <= 1e-12 * float(ref[t].abs().max()), (shape, nm, wrong, t, why)
                    continue
                if (shape, nm, wrong) in WGRAD_BELOW_THE_DRIFT:
                    assert float((bad64[t] - ref[t]).abs().max()) < float(floors[t].max())
                    continue
                with pytest.raises(AssertionError):
                    fb.within_budget(bad[t], yard[t], ref[t], floor_ulps=ulps[t], name=f"{wrong} {k}x{m}x{n} {nm} {t}")


@pytest.mark.parametrize("k1,k2", fb.LINEAR2_WIDTHS)
def test_linear2_cases_admit_a_column_order_running_sum_and_reject_the_wrong_evaluations(k1, k2):
    """The same for every (rows, widths, family) of tests/test_linear_fp64_gpu.py: the output accumulated in fp32 one input
    column after the other, the bias last.  Exempt: the last action piece where there is no action block (k2 = 0) or the inputs
    are zero."""
    c2 = k1 + fb.LINEAR2_ID_COLUMNS
    cases = [(rows, nm, fam) for rows in fb.LINEAR2_ROWS for nm, fam in fb.linear2_case(rows, k1, k2).items()]
    for nm in fb.LINEAR2_FAMILIES:
        mine = [(rows, fam) for rows, name, fam in cases if name == nm]
        for rows, fam in mine:
            bias, x1, x2, W = fam.inputs
            xs = th.cat((x1, x2), 1)
            ws = th.cat((W[:, :k1], W[:, c2:]), 1)
            run = th.zeros(rows, 64)
            for c in range(k1 + k2):
                run = run + xs[:, c, None] * ws[None, :, c]
            run = run + bias
            ref = fb.linear2_plain(bias.double(), x1.double(), x2.double(), W.double(), 0, c2)
            yard = fb.linear2_plain(bias, x1, x2, W, 0, c2)
            assert bool(ref.isfinite().all())                           # the NaN id columns of W are skipped
            floor = fb.linear2_sum_rounding(x1, x2, W, 0, c2, fam.params.get("split"))
            ulps = fb.floor_ulps(floor, ref)
            fb.within_budget(run, yard, ref, floor_ulps=ulps, name=f"running sum {rows}x({k1}+{k2}) {nm} (floor {ulps:.0f} ulps)")
            if nm == "zero_x":
                assert th.equal(yard, bias.expand(rows, 64))
            for wrong in fb.LINEAR2_WRONG:
                bad = fb.linear2_plain(bias, x1, x2, W, 0, c2, wrong=wrong)
                if wrong == "drop_last_action_piece" and (k2 == 0 or nm == "zero_x"):
                    assert th.equal(bad, yard)
                    continue
                with pytest.raises(AssertionError):
                    fb.within_budget(bad, yard, ref, floor_ulps=ulps, name=f"{wrong} {rows}x({k1}+{k2}) {nm}")


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/optim.hip and the scalar mean of csrc/tdloss.hip: the step, layouts, families and bound of tests/test_optim_fp64_gpu.py

def _torch_step(fam, dtype, **kw):
    """clip_grad_norm_ + RMSprop.step() on copies of a family's tensors in ``dtype``, the state put where PyTorch keeps it."""
    from torch.optim import RMSprop
    p, g, v = ([t.to(dtype).clone() for t in ts] for ts in fam.inputs)
    opt = RMSprop(p, lr=fb.OPTIM_LR, alpha=fb.OPTIM_ALPHA, eps=fb.OPTIM_EPS, **kw)
    for pi, gi, vi in zip(p, g, v):
        pi.grad = gi
        opt.state[pi] = {"step": th.zeros((), dtype=th.float32), "square_avg": vi}
    norm = th.nn.utils.clip_grad_norm_(p, fam.params["max_norm"])
    opt.step()
    assert all(float(opt.state[pi]["step"]) == 1.0 for pi in p)
    return {"norm": norm, "param": p, "grad": g, "square_avg": v}


def test_optim_layouts_are_the_issues():
    lay = fb.optim_layouts()
    assert list(lay) == ["one", "sixteen_ones", "actor", "critic", "threads-1", "threads", "threads+1", "pass-1", "pass", "pass+1",
                         "three_passes", "cap"]
    total = {k: sum(v) for k, v in lay.items()}
    assert total["actor"] == 34948 and total["critic"] == 52097 and total["three_passes"] == 140017
    assert (total["pass-1"], total["pass"], total["pass+1"]) == (65535, 65536, 65537) and lay["pass+1"][-1] == 1
    assert lay["pass+1"] == [1, 16383, 7, 49145, 1] and lay["pass-1"][-1] == 49144
    assert total["cap"] == 2 ** 20 and len(lay["cap"]) == 16 and len(lay["sixteen_ones"]) == 16
    assert set(fb.OPTIM_FAMILY_LAYOUTS) <= set(lay)


@pytest.mark.parametrize("layout", ["sixteen_ones", "actor", "pass+1"])
@pytest.mark.parametrize("family", ["plain", "warm", "clip_margin", "zero_warm"])
def test_clip_rmsprop_plain_is_the_two_pytorch_calls(layout, family):
    """In fp64, to 1e-12 of each tensor's scale, against the single-tensor form of the optimiser (capturable False); max_norm
    0 and -1 are PyTorch's formula too; nothing handed in is modified."""
    fam = fb.optim_case(layout)[family]
    for max_norm in (fam.params["max_norm"], 0.0, -1.0):
        fam = fam._replace(params={"max_norm": max_norm})
        before = [[t.clone() for t in ts] for ts in fam.inputs]
        mine, want = fb.optim_run(fam, th.float64), _torch_step(fam, th.float64, capturable=False, foreach=False)
        assert all(th.equal(a, b) for xs, ys in zip(fam.inputs, before) for a, b in zip(xs, ys))
        assert abs(float(mine["norm"] - want["norm"])) <= 1e-12 * float(want["norm"])
        for key in ("param", "grad", "square_avg"):
            for a, b in zip(mine[key], want[key]):
                assert a.dtype == th.float64 and float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), fb.TINY), (key, max_norm)
        if max_norm <= 0:                           # zero, or turned round
            assert all(float((a - max_norm * b.double() / (mine["norm"] + 1e-6)).abs().max()) < 1e-12 for a, b in zip(mine["grad"], fam.inputs[1]))


def test_optim_families_are_what_they_say():
    for layout in fb.OPTIM_FAMILY_LAYOUTS:
        fams = fb.optim_case(layout)
        assert tuple(fams) == fb.OPTIM_FAMILIES
        norm = {k: float(th.cat(f.inputs[1]).double().norm()) for k, f in fams.items()}
        print(f"optim families {layout}: " + " ".join(f"{k}={v:.4g}" for k, v in norm.items()))
        assert norm["inactive"] < fams["inactive"].params["max_norm"] == 1.0
        assert norm["plain"] > 1.0 and norm["warm"] > 1.0 and fams["plain"].params["max_norm"] == 1.0
        assert fams["clip_margin"].params["max_norm"] == 1e-3 and abs(norm["clip_margin"] - 2e-3) < 1e-8
        assert norm["zero"] == 0.0 == norm["zero_warm"]
        for k, f in fams.items():
            p, g, v = f.inputs
            assert all(t.dtype == th.float32 for ts in f.inputs for t in ts) and [t.numel() for t in g] == fb.optim_layouts()[layout]
            assert all(th.equal(a, b) for a, b in zip(p, fams["plain"].inputs[0]))
            zero_state = k in ("plain", "tiny", "zero")
            assert all(bool((t == 0).all()) == zero_state for t in v if t.numel() > 8)
        # the coefficient of the inactive family is exactly 1 in fp32, so the gradients keep their bits
        assert all(th.equal(a, b) for a, b in zip(fb.optim_run(fams["inactive"], th.float32)["grad"], fams["inactive"].inputs[1]))
        tiny = fb.optim_run(fams["tiny"], th.float64)["square_avg"]
        assert max(float(t.max()) for t in tiny) ** 0.5 < 0.1 * fb.OPTIM_EPS
    # norm_first_pass_only leaves out one element of pass+1 — the last tensor: it must weigh enough to be seen in the norm
    last = float(fb.optim_case("pass+1")["plain"].inputs[1][-1])
    assert abs(last) > 0.5, last
    # large: the fp32 sum of squares over the 2^20 elements of the cap is finite, and so are the squares of warm's state
    large = fb.optim_case("cap")["large"]
    flat = th.cat(large.inputs[1])
    assert flat.numel() == 2 ** 20 and flat.dtype == th.float32
    ss = (flat * flat).sum(dtype=th.float32)
    assert bool(th.isfinite(ss)) and float(ss) > 1e35 and bool(th.isfinite(th.cat(large.inputs[2])).all())


@pytest.mark.parametrize("layout", fb.OPTIM_FAMILY_LAYOUTS)
def test_the_fp32_step_passes_its_own_budget_in_every_optim_family(layout):
    """``clip_rmsprop_plain`` in fp32 in the kernel's place, PyTorch's two calls in fp32 the yardstick (MARGIN and FLOOR_ULPS as
    they stand), and the other way round."""
    for name, fam in fb.optim_case(layout).items():
        ref, plain, yard = fb.optim_run(fam, th.float64), fb.optim_run(fam, th.float32), _torch_step(fam, th.float32)
        fb.optim_within_budget(plain, yard, ref, name=f"optim plain-as-kernel {layout} {name}")
        fb.optim_within_budget(yard, plain, ref, name=f"optim torch-as-kernel {layout} {name}")
        if name == "zero":
            assert all(th.equal(a, b) for key, k in (("param", 0), ("square_avg", 2)) for a, b in zip(yard[key], fam.inputs[k]))


OPTIM_REJECTED = {"eps_inside_root": ("plain", "param"), "v_from_unclipped": ("plain", "square_avg"), "no_margin": ("clip_margin", "grad"),
                  "per_tensor_clip": ("plain", "grad"), "norm_first_pass_only": ("plain", "norm")}


@pytest.mark.parametrize("wrong", fb.OPTIM_WRONG)
def test_budget_rejects_five_wrong_optimiser_steps(wrong):
    """Each wrong evaluation in fp32 in the kernel's place, at the (family, tensor kind) where it must show: at least one tensor
    of that kind is outside the budget.  norm_first_pass_only differs from the step only past 65 536 flat elements: at pass+1
    (one element left out) and three_passes; the others at the three layouts every family runs at."""
    family, kind = OPTIM_REJECTED[wrong]
    assert set(OPTIM_REJECTED) == set(fb.OPTIM_WRONG)
    layouts = ("pass+1", "three_passes") if wrong == "norm_first_pass_only" else fb.OPTIM_FAMILY_LAYOUTS
    for layout in layouts:
        fam = fb.optim_case(layout)[family]
        ref, yard, bad = fb.optim_run(fam, th.float64), _torch_step(fam, th.float32), fb.optim_run(fam, th.float32, wrong=wrong)
        if kind == "norm":
            _rejected(bad["norm"], yard["norm"], ref["norm"], f"optim {wrong} {layout} {family} norm")
            continue
        outside = 0
        for t, (b, y, r) in enumerate(zip(bad[kind], yard[kind], ref[kind])):
            try:
                fb.within_budget(b, y, r, name=f"optim {wrong} {layout} {family} {kind}[{t}]")
            except AssertionError:
                outside += 1
        assert outside >= 1, (wrong, layout)
    if wrong == "norm_first_pass_only":             # inside the first trip there is nothing to lose
        fam = fb.optim_case("actor")[family]
        assert th.equal(fb.optim_run(fam, th.float32, wrong=wrong)["norm"], fb.optim_run(fam, th.float32)["norm"])


@pytest.mark.parametrize("kind", fb.MEAN_INPUTS)
def test_the_bound_of_a_mean_admits_an_fp64_sum_and_rejects_an_fp32_running_sum(kind):
    """``mean_within_bound`` at every size of tests/test_optim_fp64_gpu.py: a sum held in fp64 in blocks of 256 (any order
    will do) with the scale and the result rounded to fp32 is inside it; at 100 003 elements of randn + 1000 an fp32 running sum
    is outside it (partial sums of 1e8 carry roundings of 4 each)."""
    g = th.Generator().manual_seed(11)
    for n in fb.MEAN_SIZES:
        x = fb.mean_input(kind, n, g)
        for sign in (1.0, -1.0):
            pad = th.cat((x.double(), th.zeros(-n % 256, dtype=th.float64))).view(-1, 256).sum(1)
            scale = th.tensor(sign / n, dtype=th.float32).double()
            fb.mean_within_bound((pad.flip(0).sum() * scale).float(), x, sign, name=f"fp64 blocks {kind} n={n} sign={sign:+.0f}")
    if kind == "randn+1000":
        x = fb.mean_input(kind, 100003, g)
        import numpy as np
        sums = np.add.accumulate(x.numpy(), dtype=np.float32)           # one fp32 addition after the other
        seq = th.zeros((), dtype=th.float32)
        for value in x[:4096]:
            seq = seq + value
        assert float(seq) == float(sums[4095])
        with pytest.raises(AssertionError):
            fb.mean_within_bound(th.tensor(sums[-1]) / 100003, x, name="fp32 running sum randn+1000 n=100003")
