"""The QMIX mixer's kernels (csrc/qmix.hip through nets.QMixer.forward, with the flexnet_wgrad reductions of its backward)
against the fp64 copy of the mixer through tests/fp64_budget.py's ``qmix_plain``, on that module's error budget and the
mixer's input families, at the shapes where the tile scheme, the state's k-loop and the host's chunking of d_w1 take another
path; then what needs no tolerance — a launch's samples do not depend on their neighbours, on their order, on whether h1 is
saved or on the state's row stride — and the rule for a diverged run: a NaN that the PyTorch composition reports, the fused
node reports too.  Bias gradients are sums over the batch of terms that cancel: one that misses the plain budget is held to
fb.row_sum_rounding's floor instead, and the run says which.  The figures of a run are filed in
profiles/fp64_error_budget.txt."""
import copy
import functools

import pytest
import torch as th

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

# (B, n, obs_size), S = n obs_size
SHAPES = [(1, 1, 16),        # one sample in one lane; the smallest state (the k-loop runs twice)
          (32, 2, 24),       # a full tile; S = 48, an odd number of 16-column groups
          (33, 8, 16),       # a tile plus one sample; eight agents: d_w1 in 160 + 160 + 160 + 32 columns
          (31, 3, 16),       # a partial tile; 160 + 32 columns
          (129, 5, 144),     # the shipped state; one sample alone in a second work-group (4 x 32 samples each)
          (300, 8, 128)]     # S = 1024, the largest
FAMILIES = fb.QMIX_FAMILIES
STRUCTURE = [(129, 5, 144), (33, 8, 16)]
NAN_WEIGHTS = [("hyper_w_1.0.weight", (5, 7)), ("V.0.bias", (3,)), ("hyper_w_final.0.bias", (0,))]


def case_inputs(B, n, obs, family, device, attempts=32):
    """(mixer, agent_qs [B, n], states [B, S], w [B] with the tied samples' weights zeroed, tie share, attempt) on ``device``.
    Everything is drawn on the CPU (the same numbers wherever the case then runs).  One tied sample of 31 is 3.2 %, and in
    the reset and dead families every sample has the same pre-activations: the seed is chosen — the first attempt whose tie
    share is within fb.TIE_CAP, a condition on the inputs found in fp64 before any kernel runs
    (tests/test_fp64_budget_cpu.py holds it for every case)."""
    for attempt in range(attempts):
        g = th.Generator().manual_seed(100000 * attempt + 1000 * B + 10 * obs + n)
        fam = fb.qmix_families(B, n, n * obs, g)[family]
        mixer = fb.apply_params(fb.make_mixer(n, obs, seed=attempt, zero_rows="zero_rows" in fam.params), fam)
        q, x, w = fam.inputs
        share = fb.qmix_clear_ties(fb.ref64(mixer), x, w)
        if share <= fb.TIE_CAP:
            break
    else:
        raise AssertionError(f"no draw of {family} {B}x{n}x{obs} within the tie cap in {attempts} attempts")
    return mixer.to(device), q.to(device), x.to(device), w.to(device), share, attempt


@functools.lru_cache(maxsize=None)
def _case(B, n, obs, family):
    """The case on the GPU with its yardstick and its reference (fb.qmix_run), computed once and left unchanged."""
    m, q, x, w, share, _ = case_inputs(B, n, obs, family, "cuda")
    return m, q, x, w, share, fb.qmix_run(m, q, x, w, th.float32), fb.qmix_run(fb.ref64(m), q, x, w, th.float64)


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The cached cases hold GPU tensors: let them go with this file."""
    yield
    _case.cache_clear()
    th.cuda.empty_cache()


def fused(m, q, x, w, param_grads=True):
    """One pass through QMixer.forward on the HIP path: (q_tot [B], d agent_qs, {name: .grad or None})."""
    from safe_marl_amd import util
    util.FALLBACKS.pop("qmix", None)
    assert m.fused_supported(q, x)
    qq = q.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    y = m(qq, x, param_grads=param_grads)
    assert "qmix" not in util.FALLBACKS and y.shape == (q.shape[0], 1, 1)
    (y.view(-1) * w).sum().backward()
    return y.detach().view(-1), qq.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


def _held(got, t32, ref, floor, name):
    """fb.within_budget; a bias gradient (``floor`` its fb.row_sum_rounding) that misses it is held with that floor, and says so."""
    try:
        return fb.within_budget(got, t32, ref, name=name)
    except AssertionError:
        if floor is None:
            raise
    print(f"fp64-budget {name}: over the plain budget, held to the row_sum_rounding floor "
          f"({fb.floor_ulps(floor, ref) - fb.FLOOR_ULPS:.1f} ulps of its scale)")
    return fb.within_budget(got, t32, ref, floor_ulps=fb.floor_ulps(floor, ref), name=name + " [row-sum floor]")


@pytest.mark.parametrize("B,n,obs", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_forward_and_backward_within_budget(family, B, n, obs):
    m, q, x, w, share, t32, r64 = _case(B, n, obs, family)
    assert share <= fb.TIE_CAP
    y, dq, grads = fused(m, q, x, w)
    tag = f"qmix {family} {B}x{n}x{obs}"
    assert th.isfinite(y).all() and th.isfinite(dq).all() and all(th.isfinite(g).all() for g in grads.values()), tag
    fb.within_budget(y, t32[0], r64[0], name=f"{tag} q_tot")
    if family == "elu_deep":      # d agent_qs of 1e-39 .. 1e-242 in the reference: no relative comparison means anything
        return
    fb.within_budget(dq, t32[1], r64[1], name=f"{tag} d_agent_qs")
    assert set(grads) == set(r64[2]) and len(grads) == 14
    for name, g64 in r64[2].items():
        _held(grads[name], t32[2][name], g64, r64[3].get(name), f"{tag} d_{name}")
    zero = th.zeros((), device="cuda")
    if family == "reset":         # d W = d_pre^T 0
        for name in ("hyper_w_1.0.weight", "hyper_w_final.0.weight", "V.0.weight", "hyper_b_1.weight"):
            assert not r64[2][name].any() and th.equal(grads[name], zero.expand_as(grads[name])), (tag, name)
    if family == "dead":          # every hidden unit of the three ReLU heads off
        for head in fb.QMIX_RELU_HEADS:
            for name in (f"{head}.0.weight", f"{head}.0.bias"):
                assert not r64[2][name].any() and th.equal(grads[name], zero.expand_as(grads[name])), (tag, name)
    if family == "zeros":         # sign(0) = 0 through abs: nothing into the zeroed rows
        for head, step in (("hyper_w_1", 7), ("hyper_w_final", 5)):
            for name in (f"{head}.2.weight", f"{head}.2.bias"):
                rows = grads[name][::step]
                assert not r64[2][name][::step].any() and th.equal(rows, zero.expand_as(rows)), (tag, name)


# ---------------------------------------------------------------------------------------------------------------------------
# structure, bit for bit: the kernels have no communication between samples but other_half

@pytest.mark.parametrize("B,n,obs", STRUCTURE)
def test_a_prefix_of_a_launch_is_the_launch_on_the_prefix(B, n, obs):
    """What a partial last tile's lanes, which re-read row batch - 1, could break."""
    m, q, x, w = _case(B, n, obs, "plain")[:4]
    y, dq, _ = fused(m, q, x, w)
    for part in (1, 31, 32, 33, 128):
        if part >= B:
            continue
        yp, dqp, _ = fused(m, q[:part], x[:part], w[:part])
        assert th.equal(yp, y[:part]) and th.equal(dqp, dq[:part]), part


@pytest.mark.parametrize("B,n,obs", STRUCTURE)
def test_a_permutation_of_the_samples_permutes_the_outputs(B, n, obs):
    m, q, x, w = _case(B, n, obs, "plain")[:4]
    y, dq, _ = fused(m, q, x, w)
    perm = th.randperm(B, generator=th.Generator().manual_seed(B)).cuda()
    yp, dqp, _ = fused(m, q[perm], x[perm], w[perm])
    assert th.equal(yp, y[perm]) and th.equal(dqp, dq[perm])


def test_forward_without_h1_and_the_value_step_form_give_the_full_pass_bits():
    m, q, x, w = _case(33, 8, 16, "plain")[:4]
    y, dq, grads = fused(m, q, x, w)
    assert all(g is not None for g in grads.values())
    with th.no_grad():
        assert m.fused_supported(q, x)
        assert th.equal(m(q, x).view(-1), y)                               # h1 NULL
    y2, dq2, grads2 = fused(m, q, x, w, param_grads=False)
    assert th.equal(y2, y) and th.equal(dq2, dq) and all(g is None for g in grads2.values())


@pytest.mark.parametrize("B,n,obs", [(33, 8, 16), (1, 1, 16)])
def test_a_row_strided_state_gives_the_bits_of_its_contiguous_copy(B, n, obs):
    """A row stride that is a multiple of four floats on a 16-byte aligned base is read in place (ld_state > S); every other
    layout goes through a copy in the wrapper.  One sample has no row stride to speak of."""
    m, q, x, w = _case(B, n, obs, "plain")[:4]
    S = n * obs
    want = fused(m, q, x, w)

    def view_of(width, col0):
        wide = th.full((B, width), 7.0, device="cuda")
        wide[:, col0:col0 + S] = x
        return wide[:, col0:col0 + S]

    flat = th.full((B * S + 4,), 7.0, device="cuda")
    flat[1:1 + B * S] = x.reshape(-1)
    views = {"in place, stride S + 16": view_of(S + 16, 0), "stride S + 3": view_of(S + 3, 0),
             "base off by one float": view_of(S + 16, 1), "contiguous, base off by one float": flat[1:1 + B * S].view(B, S)}
    assert views["in place, stride S + 16"].data_ptr() % 16 == 0 and views["base off by one float"].data_ptr() % 16 == 4
    assert views["contiguous, base off by one float"].is_contiguous()
    for what, xv in views.items():
        assert th.equal(xv, x)
        got = fused(m, q, xv, w)
        assert th.equal(got[0], want[0]) and th.equal(got[1], want[1]), what
        assert all(th.equal(got[2][k], want[2][k]) for k in want[2]), what


# ---------------------------------------------------------------------------------------------------------------------------
# NaN: a diverged run must not report a finite loss (tests/test_ppo_gpu.py::test_nan_inputs_are_not_hidden)

def _composition(m, q, x, w):
    """The fp32 composition on the device, the reference of what is NaN: QMixer.forward_torch and its autograd."""
    qq = q.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    y = m.forward_torch(qq, x)
    (y.view(-1) * w).sum().backward()
    return y.detach().view(-1), qq.grad, {k: p.grad.clone() for k, p in m.named_parameters()}


def _reports_what_the_composition_reports(got, ref, tag):
    """Per tensor: where the composition's gradient holds a non-finite value, the fused node's does."""
    for name, g0 in [("agent_qs", ref[1])] + list(ref[2].items()):
        g = got[1] if name == "agent_qs" else got[2][name]
        print(f"nan-report {tag} d_{name}: composition finite {bool(th.isfinite(g0).all())}, fused finite {bool(th.isfinite(g).all())}")
    for name, g0 in [("agent_qs", ref[1])] + list(ref[2].items()):
        g = got[1] if name == "agent_qs" else got[2][name]
        if not th.isfinite(g0).all():
            assert not th.isfinite(g).all(), (tag, name)


@pytest.mark.parametrize("B,n,obs", STRUCTURE)
def test_a_nan_in_the_state_reaches_its_sample_and_no_other(B, n, obs):
    m, q, x, w = _case(B, n, obs, "plain")[:4]
    clean = fused(m, q, x, w)
    bad = x.clone()
    bad[5, 3] = float("nan")
    got = fused(m, q, bad, w)
    others = th.arange(B, device="cuda") != 5
    assert th.isnan(got[0][5]) and th.equal(got[0][others], clean[0][others])
    assert th.equal(th.isnan(got[0]), th.isnan(_composition(m, q, bad, w)[0]))
    _reports_what_the_composition_reports(got, _composition(m, q, bad, w), f"state {B}x{n}x{obs}")


@pytest.mark.parametrize("B,n,obs", STRUCTURE)
@pytest.mark.parametrize("name,index", NAN_WEIGHTS, ids=[k for k, _ in NAN_WEIGHTS])
def test_a_nan_in_a_relu_heads_first_layer_is_not_hidden(name, index, B, n, obs):
    """One NaN element of a first-layer weight or bias of a ReLU head, as after a diverged step: it reaches q_tot only through
    that head's ReLU (a NaN in the state also travels by the linear hyper_b_1 head and would show either way)."""
    m0, q, x, w = _case(B, n, obs, "plain")[:4]
    m = copy.deepcopy(m0)
    with th.no_grad():
        dict(m.named_parameters())[name][index] = float("nan")
    ref = _composition(m, q, x, w)
    got = fused(m, q, x, w)
    print(f"nan-report {name} {B}x{n}x{obs} q_tot: composition NaN in {int(th.isnan(ref[0]).sum())} of {B}, "
          f"fused NaN in {int(th.isnan(got[0]).sum())}")
    assert th.isnan(ref[0]).any()
    assert th.equal(th.isnan(got[0]), th.isnan(ref[0]))
    with th.no_grad():
        assert th.equal(th.isnan(m(q, x).view(-1)), th.isnan(ref[0]))        # the forward that saves no h1
    _reports_what_the_composition_reports(got, ref, f"{name} {B}x{n}x{obs}")
