"""COMA's counterfactual baseline (csrc/coma.hip: nets.coma_baseline) against the fp64 copy of the critic, on
tests/fp64_budget.py's error budget and its ``z`` input families — the kernel takes fc1's pre-activation directly, so the rows
whose 64 LayerNorm inputs are all equal, or offset by 70 times their spread, are fed as they are.  One draw of every case is
the action taken itself, so that the sampled pass sees those rows too.  Without LayerNorm there is no ``ln_b`` to make the
``dead`` family from; the other five run.  The figures of a run are filed in profiles/fp64_error_budget.txt."""
import functools

import pytest
import torch as th

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

# (b, n, act_dim, s): a full 32-row tile and one that holds a single row (33), more than one tile per agent with a partial last
# one (77, 65), exactly one tile (32); an odd act_dim (the c < ad padding of the half-lane split), act_dim 1 (half 1 is empty)
SHAPES = [(33, 5, 4, 3), (77, 3, 4, 1), (65, 5, 3, 2), (32, 3, 1, 3)]
FAMILIES = ("plain", "reset", "offset", "constant", "dead", "mixed")
OBS = 6


def case_inputs(b, n, act_dim, s, layernorm, family, device):
    """(critic, family, z1 [b n, 64], act [b, n, a], sampled [s, b, n, a]) of a case (forward only: no tie to clear)."""
    g = th.Generator(device=device).manual_seed(1000 * b + 10 * n + act_dim + s)
    fam = fb.families(b * n, n, None, g)[family]
    critic = fb.make_critic(layernorm, device, seed=b + n, in_features=(n + 1) * OBS + n + n * act_dim)
    fb.apply_params(critic, fam)
    act = th.rand(b, n, act_dim, device=device, generator=g)
    sampled = act.unsqueeze(0) + th.randn(s, b, n, act_dim, device=device, generator=g)
    sampled[0] = act                                       # the update is 0 w in every MFMA step: q_sampled[0] is the values
    return critic, fam, fam.inputs[0], act, sampled


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The cached cases hold GPU tensors: let them go with this file."""
    yield
    _case.cache_clear()
    th.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _case(b, n, act_dim, s, layernorm, family):
    critic, fam, z1, act, sampled = case_inputs(b, n, act_dim, s, layernorm, family, "cuda")
    c64 = fb.ref64(critic)
    with th.no_grad():
        t32 = fb.coma_baseline_plain(critic, z1, act, sampled)[:3]
        r64 = fb.coma_baseline_plain(c64, z1.double(), act.double(), sampled.double())[:3]
    return critic, fam, z1, act, sampled, t32, r64


def _rows(t, mask):
    """baseline / values [b, n] or q_sampled [s, b, n] on the rows (b, i) of ``mask`` [b n]."""
    return t.reshape(-1, mask.numel())[:, mask]


@pytest.mark.parametrize("b,n,act_dim,s", SHAPES)
@pytest.mark.parametrize("layernorm,family", [(True, f) for f in FAMILIES] + [(False, f) for f in FAMILIES if f != "dead"])
def test_baseline_within_budget(layernorm, family, b, n, act_dim, s):
    from safe_marl_amd import util
    from safe_marl_amd.nets import coma_baseline
    critic, fam, z1, act, sampled, t32, r64 = _case(b, n, act_dim, s, layernorm, family)
    util.FALLBACKS.pop("coma", None)
    out = coma_baseline(critic, z1, act, sampled, want_q=True, want_values=True)
    assert "coma" not in util.FALLBACKS                                      # the HIP launch, not the tensor form
    tag = f"coma_baseline {family} ln={int(layernorm)} {b}x{n}x{act_dim}x{s}"
    every = th.ones(b * n, dtype=th.bool, device="cuda")
    groups = [("", every)]
    if fam.groups is not None:
        groups += [(f"[{nm} rows]", fam.groups == j) for j, nm in enumerate(fb.MIXED_OF["z"])]
    for sub, mask in groups:
        for k, nm in enumerate(("baseline", "q_sampled", "values")):
            assert th.isfinite(out[k]).all(), (tag, nm)
            fb.within_budget(_rows(out[k], mask), _rows(t32[k], mask), _rows(r64[k], mask), name=f"{tag} {nm}{sub}")
    assert th.equal(out[1][0], out[2])                     # the draw that is the action taken: the values, bit for bit
    # the last sample, which a partial last tile reads again for its dead lanes: within the whole batch's budget above, and
    # the very bits of a launch on that sample alone (a row's arithmetic does not depend on its place in a tile)
    alone = coma_baseline(critic, z1[-n:], act[-1:], sampled[:, -1:], want_q=True, want_values=True)
    assert th.equal(alone[0], out[0][-1:]) and th.equal(alone[1], out[1][:, -1:]) and th.equal(alone[2], out[2][-1:])
    only, none_q, none_v = coma_baseline(critic, z1, act, sampled)
    assert none_q is None and none_v is None and th.equal(only, out[0])
