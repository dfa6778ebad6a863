"""The shared RNN actor's kernels (csrc/actor.hip, actor_r16.h, gru.hip, lnrelu.hip, wgrad.hip, reached through nets) against
the fp64 evaluation of nets.RNNAgent, on tests/fp64_budget.py's error budget and input families: the inference launch in its
four variants, one NaN row among finite ones, the fused training node under both backward forms, and csrc/lnrelu.hip's node
on its own.  The figures of a run are filed in profiles/fp64_error_budget.txt."""
import functools
import types

import pytest
import torch as th

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

STD = 0.75                                          # exact in fp32: the kernel's std is the reference's
FWD_SHAPES = [(13, 5, 144, 4), (7, 3, 72, 2), (130, 8, 6, 8)]     # 65 rows: a partial 16-row tile and a partial 32-row tile
FWD_CASES = [(f, True) for f in ("plain", "reset", "offset", "saturated", "dead", "mixed")] + [("plain", False), ("saturated", False)]
TRAIN_SHAPES = [(2565, 5, 144, 4), (2052, 3, 72, 2), (2056, 8, 6, 8)]   # >= WGRAD_MIN_ROWS, the last 16-row tile not full
TRAIN_FAMILIES = ("plain", "reset", "offset", "saturated", "dead", "mixed")
ACTION_ARGS = types.SimpleNamespace(continuous=True, action_low=0.0, action_high=1.0)


def _explore(means, noise):
    """util.py:57-64, 121-130 in the dtype of ``means``: action = tanh(mean + std noise), and what the environment is handed."""
    from safe_marl_amd.util import translate_action
    action = th.tanh(means + STD * noise.to(means.dtype))
    env = th.from_numpy(translate_action(ACTION_ARGS, action, None)[1]).to(means.device).view_as(action)
    return action, env


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The cached cases hold GPU tensors: let them go with this file."""
    yield
    _forward_case.cache_clear()
    th.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _forward_case(b, n, obs_dim, act, family, ln):
    """Agent, inputs and the two references of one forward case, computed once for the four kernel variants."""
    rows = b * n
    g = th.Generator(device="cuda").manual_seed(rows + act)
    fam = fb.families(rows, n, obs_dim, g)[family]
    agent = fb.apply_params(fb.make_agent(obs_dim, n, act, layernorm=ln, device="cuda"), fam)
    obs, hid = fam.inputs
    noise = th.randn(rows, act, device="cuda", generator=g)
    flat = noise.view(-1)
    flat[::5] = 20.0 / STD                          # std * noise = +-20: past fast_tanh's clamp at 15
    flat[::10] = -20.0 / STD
    with th.no_grad():
        t32 = fb.actor_plain(agent, obs, hid, n)[:2]
        t32 = t32 + _explore(t32[0], noise)
        a64 = fb.ref64(agent)
        r64 = fb.actor_plain(a64, obs.double(), hid.double(), n)[:2]
        r64 = r64 + _explore(r64[0], noise)
    # rows with saturated gates: each output's floor is 8 ulps plus fb.gate_rounding's figure (derived there) for the element of
    # that tensor that hangs most on a gate in transition
    wide = fb.gate_rounding(a64, obs.double(), hid.double(), n, noise, STD) if family in ("saturated", "mixed") else None
    return agent, fam, noise, t32, r64, wide


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("b,n,obs_dim,act", FWD_SHAPES)
@pytest.mark.parametrize("family,ln", FWD_CASES)
def test_inference_launch_within_budget(family, ln, b, n, obs_dim, act, variant):
    from safe_marl_amd.nets import fused_actor_forward
    agent, fam, noise, t32, r64, wide = _forward_case(b, n, obs_dim, act, family, ln)
    obs, hid = fam.inputs
    out = fused_actor_forward(agent, obs.view(b, n, obs_dim), hid, n, True, noise=noise.view(b, n, act), std=STD, low=0.0,
                              high=1.0, variant=variant)
    assert out is not None
    tag = f"actor_forward[v{variant}] {family}{'' if ln else '-noln'} {b}x{n}x{obs_dim}x{act}"
    groups = [("", slice(None))]
    if fam.groups is not None:                      # a reset or saturated row must not change its tile neighbours: each kind alone
        groups += [(f"[{nm} rows]", fam.groups == j) for j, nm in enumerate(fb.MIXED_OF["actor"])]
    for sub, rows in groups:
        for k, nm in enumerate(("means", "hidden", "action", "env_action")):
            assert th.isfinite(out[k][rows]).all(), (tag, nm)
            floor = fb.FLOOR_ULPS
            if wide is not None and sub in ("", "[saturated rows]"):       # (the plain and reset rows of a mixed batch: 8 ulps)
                floor += float(wide[nm][rows].max()) / (fb.ULP * float(r64[k][rows].abs().max()))
            fb.within_budget(out[k][rows], t32[k][rows], r64[k][rows], floor_ulps=floor, name=f"{tag} {nm}{sub}")


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("row", [32, 64, 37], ids=["first-of-tile", "last-of-batch", "middle"])
def test_one_nan_row_stays_in_its_row(row, variant):
    """A row of NaN observations (no fault: the kernels compute no address from data) gives NaN outputs for that row, as the
    module does, and leaves every other row — its tile neighbours, and the rows a partial tile re-reads — bit for bit what it
    is with that row zeroed."""
    from safe_marl_amd.nets import fused_actor_forward
    b, n, obs_dim, act = FWD_SHAPES[0]
    agent, fam, noise, _, _, _ = _forward_case(b, n, obs_dim, act, "plain", True)
    obs, hid = fam.inputs
    outs = []
    for fill in (float("nan"), 0.0):
        o = obs.clone()
        o[row] = fill
        outs.append(fused_actor_forward(agent, o.view(b, n, obs_dim), hid, n, True, noise=noise.view(b, n, act), std=STD,
                                        low=0.0, high=1.0, variant=variant))
    others = th.arange(b * n, device="cuda") != row
    for nm, bad, zeroed in zip(("means", "hidden", "action", "env_action"), *outs):
        assert th.isnan(bad[row]).all(), nm
        assert th.equal(bad[others], zeroed[others]), nm


@pytest.mark.parametrize("fused_bwd", [True, False], ids=["gru-bwd-fused", "gru-bwd-composed"])
@pytest.mark.parametrize("rows,n,obs_dim,act", TRAIN_SHAPES)
@pytest.mark.parametrize("family", TRAIN_FAMILIES)
def test_training_node_within_budget(family, rows, n, obs_dim, act, fused_bwd, monkeypatch):
    """RNNAgent.forward_update through the fused node, a gradient fed into the means AND the new hidden state (the node the
    Gaussian agent uses: nets._ActorTrainHidFn)."""
    from safe_marl_amd import nets
    monkeypatch.setattr(nets, "GRU_BWD_FUSED", fused_bwd)
    g = th.Generator(device="cuda").manual_seed(rows + n)
    fam = fb.families(rows, n, obs_dim, g)[family]
    agent = fb.apply_params(fb.make_agent(obs_dim, n, act, device="cuda"), fam)
    obs, hid = fam.inputs
    up = [th.randn(rows, act, device="cuda", generator=g) / rows, th.randn(rows, 64, device="cuda", generator=g) / rows]
    a64 = fb.ref64(agent)
    assert fb.clear_ties(a64, (obs.double(), hid.double(), n), up) <= fb.TIE_CAP
    agent.fused_training = True
    agent._train_node = lambda: nets._ActorTrainHidFn
    assert nets.actor_train_supported(agent, obs, n, True)

    def fused():
        means, _, h = agent.forward_update(obs, hid, n, True)
        assert "ActorTrainHidFn" in type(means.grad_fn).__name__ and h.requires_grad
        return means, h

    kern = fb.run_with_grads(fused, dict(agent.named_parameters()), up)
    t32 = fb.run_with_grads(lambda: fb.actor_plain(agent, obs, hid, n)[:2], dict(agent.named_parameters()), up)
    r64 = fb.run_with_grads(lambda: fb.actor_plain(a64, obs.double(), hid.double(), n)[:2], dict(a64.named_parameters()),
                            [u.double() for u in up])
    tag = f"actor_train[{'fused' if fused_bwd else 'composed'} bwd] {family} {rows}x{n}x{obs_dim}x{act}"
    for k, nm in enumerate(("means", "hidden")):
        fb.within_budget(kern[0][k], t32[0][k], r64[0][k], name=f"{tag} {nm}")
    for nm, g64 in r64[1].items():
        assert th.isfinite(kern[1][nm]).all(), (tag, nm)
        if family == "dead" and nm in ("fc1.weight", "fc1.bias", "layernorm.weight"):
            assert not g64.any() and not kern[1][nm].any(), (tag, nm)     # every ReLU unit off: dz rows exactly zero
        fb.within_budget(kern[1][nm], t32[1][nm], g64, name=f"{tag} d_{nm}")


@pytest.mark.parametrize("with_bias_ids", [True, False], ids=["bias-ids", "bare"])
@pytest.mark.parametrize("rows,n", [(65, 5), (7, 1), (2053 * 3, 3)])
@pytest.mark.parametrize("family", ["plain", "reset", "offset", "constant", "dead", "mixed"])
def test_lnrelu_node_within_budget(family, rows, n, with_bias_ids):
    """nets._LnReluFn (csrc/lnrelu.hip) on its own; bare, the constant family reaches LayerNorm as it is: zero variance."""
    from safe_marl_amd.nets import _LnReluFn
    g = th.Generator(device="cuda").manual_seed(rows + n)
    fam = fb.families(rows, n, None, g)[family]
    z = fam.inputs[0]
    p = {"bias": 0.3 * th.randn(64, device="cuda", generator=g) if with_bias_ids else None,
         "ids": 0.3 * th.randn(n, 64, device="cuda", generator=g) if with_bias_ids else None,
         "ln_w": 0.3 * th.randn(64, device="cuda", generator=g), "ln_b": 0.3 * th.randn(64, device="cuda", generator=g)}
    if "ln_b" in fam.params:
        p["ln_b"].fill_(fam.params["ln_b"][1])
    up = [th.randn(rows, 64, device="cuda", generator=g) / rows]
    order = ("z", "bias", "ids", "ln_w", "ln_b")
    p64 = {k: fb.cast(v) for k, v in p.items()}
    share = fb.clear_ties(lambda zz: [fb.lnrelu_plain(zz, p64["bias"], p64["ids"], p64["ln_w"], p64["ln_b"], n)[1]],
                          (z.double(),), up)
    assert share <= fb.TIE_CAP

    def run(fn, dtype):
        leaves = {"z": z.clone().to(dtype).requires_grad_(True)}
        leaves.update({k: v.clone().to(dtype).requires_grad_(True) for k, v in p.items() if v is not None})
        args = [leaves.get(k) for k in order]
        return fb.run_with_grads(lambda: (fn(*args),), leaves, [up[0].to(dtype)])

    kern = run(lambda *a: _LnReluFn.apply(*a, 1e-5, n), th.float32)
    t32 = run(lambda *a: fb.lnrelu_plain(*a, n)[0], th.float32)
    r64 = run(lambda *a: fb.lnrelu_plain(*a, n)[0], th.float64)
    tag = f"lnrelu[{'bias+ids' if with_bias_ids else 'bare'}] {family} {rows}x{n}"
    if family == "dead":
        assert not r64[0][0].any() and not kern[0][0].any() and not kern[1]["z"].any()
    fb.within_budget(kern[0][0], t32[0][0], r64[0][0], name=f"{tag} out")
    for nm, g64 in r64[1].items():
        assert th.isfinite(kern[1][nm]).all(), (tag, nm)
        fb.within_budget(kern[1][nm], t32[1][nm], g64, name=f"{tag} d_{nm}")
