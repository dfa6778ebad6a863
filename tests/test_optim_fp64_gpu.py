"""The optimiser step every sub-update ends in (csrc/optim.hip: flexnet_clip_rmsprop through optim.clip_and_step) and the scalar
mean every reported loss goes through (csrc/tdloss.hip: flexnet_scaled_sum through util.mean_all) on the fp64 error budget of
tests/fp64_budget.py.

The step: every parameter, gradient and square_avg is a slice of a sentinel-filled flat buffer at an offset that is no multiple of
four elements, the sentinels are looked at after every call, and the optimiser is a real torch.optim.RMSprop(capturable=True)
whose state the kernel moves.  The yardstick is clip_grad_norm_ + RMSprop.step() in fp32 on copies, the reference
``fb.clip_rmsprop_plain`` in fp64; ``fb.within_budget`` is applied to the norm and, tensor by tensor, to every parameter, gradient
and square_avg.  Layouts (``fb.optim_layouts``) on both sides of the 16 384 threads and of the 65 536 elements of one trip of the
kernels' loops, 16 tensors, one-element tensors, the cap of 2^20 elements; families (``fb.optim_families``) with the clip on, off
and at its margin, squares near the top of fp32, and exact zeros.  Then what must hold exactly: unchanged bits where nothing may
move, the counters, a gradient that is None, two runs, gradients that are views of one flat bucket (the trainer's multi-rank
layout), the three ways out to PyTorch, a NaN and an Inf gradient, no gradient at all, a parameter of no elements, max_norm <= 0,
and the refresh that rides in the step's launches past the first trip.

The mean: 12 sizes around the block (256), the grid (16 384) and the pair of strides (32 768) of the kernel's loop, three inputs,
both signs, against the bound ``fb.mean_within_bound`` derives; the gradient under util.unit_seed and under an ordinary one; the
floats around the output.  The figures of a run are filed in profiles/fp64_error_budget.txt."""
import pytest
import torch as th

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

SENTINEL = 3e33          # its square is beyond fp32: one sentinel read into the norm makes it inf, one overwritten changes bits
KEYS = ("norm", "param", "grad", "square_avg")
HYPER = dict(lr=fb.OPTIM_LR, alpha=fb.OPTIM_ALPHA, eps=fb.OPTIM_EPS)


class Slab:
    """Copies of ``tensors`` (flat, fp32) as slices ``views`` of ONE flat GPU buffer filled with SENTINEL: every slice starts at
    an offset that is no multiple of four elements and has at least one sentinel on either side.  ``intact()``: every sentinel
    still has its bits."""

    def __init__(self, tensors):
        offsets, off = [], 1
        for t in tensors:
            off += 1 if off % 4 == 0 else 0
            offsets.append(off)
            off += t.numel() + 1
        self.buf = th.full((off + 2,), SENTINEL, device="cuda")
        self.guard = th.ones(off + 2, dtype=th.bool, device="cuda")
        self.views = []
        for o, t in zip(offsets, tensors):
            assert o % 4 != 0
            self.views.append(self.buf[o:o + t.numel()])
            self.views[-1].copy_(t.reshape(-1))
            self.guard[o:o + t.numel()] = False

    def intact(self):
        return bool((self.buf[self.guard] == SENTINEL).all())


def _fallbacks():
    from safe_marl_amd import util
    return util.FALLBACKS.get("clip_rmsprop", 0)


def _optimizer(params, grads, square_avgs, steps=None, **kw):
    """A capturable RMSprop on ``params`` with the state put where PyTorch keeps it; a gradient that is None stays None."""
    from torch.optim import RMSprop
    opt = RMSprop(params, **{**HYPER, **kw}, capturable=True)
    for i, (p, g, v) in enumerate(zip(params, grads, square_avgs)):
        p.grad = g
        if v is not None:
            opt.state[p] = {"step": th.zeros((), device="cuda") if steps is None else steps[i].clone(), "square_avg": v}
    return opt


def _setup(fam, drop=()):
    """(optimiser, params, the three Slabs) of a family's tensors on the GPU; the tensors in ``drop`` get no gradient."""
    slabs = [Slab(ts) for ts in fam.inputs]
    params = slabs[0].views
    grads = [None if i in drop else g for i, g in enumerate(slabs[1].views)]
    return _optimizer(params, grads, slabs[2].views), params, slabs


def _snapshot(opt, params):
    """Clones of (params, grads, square_avgs, steps) of the tensors that have a gradient, and their indices."""
    live = [i for i, p in enumerate(params) if p.grad is not None]
    own = [params[i] for i in live]
    return ([p.detach().clone() for p in own], [p.grad.clone() for p in own], [opt.state[p]["square_avg"].clone() for p in own],
            [opt.state[p]["step"].clone() for p in own]), live


def _yardstick(snap, max_norm, **kw):
    """The two PyTorch calls in fp32 on (clones of) a snapshot: the result in ``fb.optim_run``'s form, with the counters."""
    p, g, v, s = ([t.clone() for t in ts] for ts in snap)
    opt = _optimizer(p, g, v, s, **kw)
    norm = th.nn.utils.clip_grad_norm_(p, max_norm)
    opt.step()
    return {"norm": norm, "param": p, "grad": g, "square_avg": v, "step": [opt.state[t]["step"] for t in p]}


def _reference(snap, max_norm):
    p, g, v = ([t.double() for t in ts] for ts in snap[:3])
    return dict(zip(KEYS, fb.clip_rmsprop_plain(p, g, v, max_norm, fb.OPTIM_LR, fb.OPTIM_ALPHA, fb.OPTIM_EPS)))


def _kernel_step(opt, params, max_norm, slabs, live):
    """One ``clip_and_step`` through the kernel (no fall-back noted), the sentinels looked at: the result in optim_run's form."""
    from safe_marl_amd.optim import clip_and_step
    noted = _fallbacks()
    norm = clip_and_step(opt, params, max_norm)
    th.cuda.synchronize()
    assert _fallbacks() == noted, "the step went to PyTorch"
    assert all(s.intact() for s in slabs), "a sentinel was overwritten"
    assert norm.dim() == 0 and norm.dtype == th.float32 and norm.is_cuda
    own = [params[i] for i in live]
    return {"norm": norm.clone(), "param": [p.detach().clone() for p in own], "grad": [p.grad.clone() for p in own],
            "square_avg": [opt.state[p]["square_avg"].clone() for p in own], "step": [opt.state[p]["step"].clone() for p in own]}


def _step_and_check(opt, params, max_norm, slabs, name):
    """Yardstick and reference from the state as it is, then the kernel's step held to the budget; the counters are PyTorch's."""
    snap, live = _snapshot(opt, params)
    yard, ref = _yardstick(snap, max_norm), _reference(snap, max_norm)
    kern = _kernel_step(opt, params, max_norm, slabs, live)
    fb.optim_within_budget(kern, yard, ref, name=name)
    assert [float(s) for s in kern["step"]] == [float(s) for s in yard["step"]] == [float(s) + 1.0 for s in snap[3]]
    return kern, yard, ref, snap


def _same_bits(a, b, keys=KEYS + ("step",)):
    for key in keys:
        xs, ys = (a[key], b[key]) if isinstance(a[key], list) else ([a[key]], [b[key]])
        assert len(xs) == len(ys)
        for t, (x, y) in enumerate(zip(xs, ys)):
            assert th.equal(x.view(th.int32) if x.dtype == th.float32 else x, y.view(th.int32) if y.dtype == th.float32 else y), (key, t)


# ---------------------------------------------------------------------------------------------------------------------------
# the budget

@pytest.mark.parametrize("family", ["plain", "warm"])
@pytest.mark.parametrize("layout", list(fb.optim_layouts()))
def test_every_layout_on_a_first_and_a_warm_step(layout, family):
    fam = fb.optim_case(layout)[family]
    opt, params, slabs = _setup(fam)
    _step_and_check(opt, params, fam.params["max_norm"], slabs, f"optim {layout} {family}")


@pytest.mark.parametrize("family", [f for f in fb.OPTIM_FAMILIES if f not in ("plain", "warm")])
@pytest.mark.parametrize("layout", fb.OPTIM_FAMILY_LAYOUTS)
def test_every_family_at_three_layouts(layout, family):
    """(plain and warm run at every layout above.)  inactive: the gradients keep their bits; zero with zero state: parameters and
    square_avg keep theirs, and nothing is NaN."""
    fam = fb.optim_case(layout)[family]
    opt, params, slabs = _setup(fam)
    kern, yard, ref, snap = _step_and_check(opt, params, fam.params["max_norm"], slabs, f"optim {layout} {family}")
    if family == "inactive":
        assert float(ref["norm"]) < fam.params["max_norm"]
        _same_bits(kern, dict(zip(KEYS[1:], snap[:3])), keys=("grad",))
    if family == "zero":
        _same_bits(kern, dict(zip(KEYS[1:], snap[:3])), keys=("param", "square_avg"))
    if family in ("zero", "zero_warm"):
        assert float(kern["norm"]) == 0.0
        assert all(bool(th.isfinite(t).all()) for key in KEYS[1:] for t in kern[key])
        _same_bits(kern, dict(zip(KEYS[1:], snap[:3])), keys=("param",))


def test_three_steps_in_a_row_and_pytorch_continues():
    """pass+1, three steps with fresh gradients (the clip on, off, on): at each the reference and the yardstick restart from the
    kernel's own state of the step before — a single-step budget each time, the counters and the state carried by the kernel
    alone.  Then state_dict() round-trips into a fresh RMSprop, whose own step() continues from it."""
    from torch.optim import RMSprop
    fam = fb.optim_case("pass+1")["plain"]
    opt, params, slabs = _setup(fam)
    g = th.Generator().manual_seed(5)
    for step, scale in enumerate((1.0, 1e-3, 5.0)):
        if step > 0:
            for view in slabs[1].views:
                view.copy_(scale * th.randn(view.numel(), generator=g))
        kern, _, _, _ = _step_and_check(opt, params, 1.0, slabs, f"optim pass+1 step {step + 1}")
        assert all(float(s) == step + 1.0 for s in kern["step"])
    sd = opt.state_dict()
    nxt = RMSprop(params, **HYPER, capturable=True)
    nxt.load_state_dict(sd)
    snap, live = _snapshot(nxt, params)
    assert live == list(range(len(params))) and all(float(s) == 3.0 for s in snap[3])
    _same_bits(dict(zip(KEYS[1:], snap[:3])), kern, keys=("square_avg",))
    want = _yardstick(snap, 1e30)                       # (a clip that is off: step() alone)
    nxt.step()
    th.cuda.synchronize()
    assert all(float(nxt.state[p]["step"]) == 4.0 for p in params)
    assert all(th.equal(p, w) for p, w in zip(params, want["param"])) and slabs[0].intact()


# ---------------------------------------------------------------------------------------------------------------------------
# exact statements

@pytest.mark.parametrize("layout,drop", [("pass+1", (4,)), ("pass+1", (0,)), ("sixteen_ones", tuple(range(1, 16, 2)))],
                         ids=["pass+1-last", "pass+1-first", "sixteen_ones-every-other"])
def test_a_tensor_without_gradient_keeps_its_bits_and_its_counter(layout, drop):
    fam = fb.optim_case(layout)["warm"]
    opt, params, slabs = _setup(fam, drop)
    before = [(params[i].clone(), opt.state[params[i]]["square_avg"].clone()) for i in drop]
    _, _, _, snap = _step_and_check(opt, params, 1.0, slabs, f"optim {layout} without {len(drop)} gradients")
    assert len(snap[0]) == len(params) - len(drop)
    for i, (p, v) in zip(drop, before):
        st = opt.state[params[i]]
        assert params[i].grad is None and th.equal(params[i], p) and th.equal(st["square_avg"], v) and float(st["step"]) == 0.0


@pytest.mark.parametrize("layout", ["pass+1", "cap"])
def test_two_runs_give_the_same_bits(layout):
    fam = fb.optim_case(layout)["warm"]
    runs = []
    for _ in range(2):
        opt, params, slabs = _setup(fam)
        runs.append(_kernel_step(opt, params, 1.0, slabs, list(range(len(params)))))
    _same_bits(*runs)


@pytest.mark.parametrize("layout", ["pass+1", "three_passes"])
def test_gradients_that_are_views_of_one_flat_bucket(layout):
    """trainer.py's multi-rank layout (``_loss_and_grads(flat=...)``): the gradients are consecutive views of one contiguous
    bucket in parameter order.  The bits of the separate-tensor run, and the bucket holds the clipped gradients."""
    fam = fb.optim_case(layout)["warm"]
    opt, params, slabs = _setup(fam)
    apart = _kernel_step(opt, params, 1.0, slabs, list(range(len(params))))
    bucket = Slab([th.cat(fam.inputs[1])])
    slabs = [Slab(fam.inputs[0]), bucket, Slab(fam.inputs[2])]
    views, off = [], 0
    for g in fam.inputs[1]:
        views.append(bucket.views[0][off:off + g.numel()])
        off += g.numel()
    opt = _optimizer(slabs[0].views, views, slabs[2].views)
    flat = _kernel_step(opt, slabs[0].views, 1.0, slabs, list(range(len(views))))
    _same_bits(flat, apart)
    assert th.equal(bucket.views[0], th.cat(apart["grad"]))


@pytest.mark.parametrize("case", ["one-element-too-many", "seventeen-tensors", "lr-is-a-tensor"])
def test_the_three_ways_out_take_the_pytorch_calls(case):
    """Past FLEXNET_OPT_MAX_ELEMENTS, past FLEXNET_OPT_MAX_TENSORS, and with a tensor for lr the step is the two PyTorch calls:
    the fall-back is noted and the bits are the yardstick's (run on slices laid out alike)."""
    from safe_marl_amd.optim import clip_and_step
    layout = {"one-element-too-many": [2 ** 20 + 1], "seventeen-tensors": [1] * 17, "lr-is-a-tensor": fb.optim_layouts()["actor"]}[case]
    fam = fb.optim_families(layout, th.Generator().manual_seed(17))["warm"]
    kw = {"lr": th.tensor(fb.OPTIM_LR, device="cuda")} if case == "lr-is-a-tensor" else {}
    res = []
    for ours in (True, False):
        slabs = [Slab(ts) for ts in fam.inputs]
        params = slabs[0].views
        opt = _optimizer(params, slabs[1].views, slabs[2].views, **kw)
        noted = _fallbacks()
        if ours:
            norm = clip_and_step(opt, params, 1.0)
            assert _fallbacks() == noted + 1
        else:
            norm = th.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
        th.cuda.synchronize()
        assert all(s.intact() for s in slabs)
        res.append({"norm": norm, "param": params, "grad": slabs[1].views, "square_avg": slabs[2].views,
                    "step": [opt.state[p]["step"] for p in params]})
    _same_bits(*res)
    assert all(float(s) == 1.0 for s in res[0]["step"])


# ---------------------------------------------------------------------------------------------------------------------------
# where clip_and_step was not the two PyTorch calls

@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_nan_and_an_inf_gradient_spread_as_pytorchs_do(value):
    """pass+1, one element of the largest tensor.  clip_grad_norm_ clamps its coefficient with torch.clamp, which hands a NaN
    on: after a NaN gradient every gradient, square_avg and parameter is NaN.  After +Inf the coefficient is 0 and only that
    element is NaN.  The NaN / Inf pattern of everything equals PyTorch's, and where PyTorch is finite the budget holds."""
    fam = fb.optim_case("pass+1")["plain"]
    opt, params, slabs = _setup(fam)
    slabs[1].views[3][30001] = value
    snap, live = _snapshot(opt, params)
    yard, ref = _yardstick(snap, 1.0), _reference(snap, 1.0)
    kern = _kernel_step(opt, params, 1.0, slabs, live)
    if value != value:
        assert all(bool(th.isnan(t).all()) for key in KEYS[1:] for t in yard[key]) and bool(th.isnan(yard["norm"]))
    else:
        assert sum(int(th.isnan(t).sum()) for t in yard["param"]) == 1 and bool(th.isinf(yard["norm"]))
    for key in KEYS:
        for t, (k, y, r) in enumerate(zip(*[[d[key]] if key == "norm" else d[key] for d in (kern, yard, ref)])):
            k, y, r = k.reshape(-1), y.reshape(-1), r.reshape(-1)
            assert th.equal(th.isnan(k), th.isnan(y)) and th.equal(th.isposinf(k), th.isposinf(y)) and th.equal(th.isneginf(k), th.isneginf(y)), (key, t)
            fin = th.isfinite(y)
            assert bool(th.isfinite(r[fin]).all())
            fb.within_budget(k[fin], y[fin], r[fin], name=f"optim pass+1 {value} gradient {key}[{t}]")
    assert [float(s) for s in kern["step"]] == [float(s) for s in yard["step"]]


def test_no_gradient_at_all_returns_zero_and_writes_nothing():
    """Every parameter's gradient is None: clip_grad_norm_ returns 0 and step() creates no state.  (The block the allocator
    hands out next is dirtied first: the number that comes back must not be whatever lay there.)"""
    from torch.optim import RMSprop
    from safe_marl_amd.optim import clip_and_step
    fam = fb.optim_case("actor")["plain"]
    slab = Slab(fam.inputs[0])
    params = slab.views
    before = slab.buf.clone()
    opt = RMSprop(params, **HYPER, capturable=True)
    for size in (1, 65, 128):
        th.full((size,), 7.0, device="cuda")
    th.cuda.synchronize()
    norm = clip_and_step(opt, params, 1.0)
    th.cuda.synchronize()
    assert th.is_tensor(norm) and norm.dim() == 0 and float(norm) == 0.0
    assert len(opt.state) == 0 and th.equal(slab.buf.view(th.int32), before.view(th.int32))
    want = th.nn.utils.clip_grad_norm_(params, 1.0)
    opt.step()
    assert want.dim() == 0 and float(want) == 0.0 and len(opt.state) == 0


def test_a_parameter_of_no_elements_is_stepped_over():
    """A (0,) parameter with a (0,) gradient among the actor's tensors: no exception, the other tensors inside the budget, and
    the empty one's state is what PyTorch leaves there."""
    from safe_marl_amd.optim import clip_and_step
    fam = fb.optim_case("actor")["warm"]
    res = []
    for ours in (True, False):
        slabs = [Slab(ts) for ts in fam.inputs]
        params, grads, states = (list(s.views) for s in slabs)
        empty = th.empty(0, device="cuda")
        assert empty.data_ptr() == 0
        params.insert(3, empty)
        grads.insert(3, th.empty(0, device="cuda"))
        states.insert(3, None)
        opt = _optimizer(params, grads, states)
        if ours:
            norm = clip_and_step(opt, params, 1.0)
        else:
            norm = th.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
        th.cuda.synchronize()
        assert all(s.intact() for s in slabs)
        full = [p for p in params if p.numel() > 0]
        res.append(({"norm": norm, "param": full, "grad": [p.grad for p in full], "square_avg": [opt.state[p]["square_avg"] for p in full]},
                    opt.state[empty], [float(opt.state[p]["step"]) for p in params]))
    ref = fb.optim_run(fam, th.float64, device="cuda")
    fb.optim_within_budget(res[0][0], res[1][0], ref, name="optim actor + a (0,) parameter")
    (_, mine, steps), (_, theirs, want) = res
    assert steps == want == [1.0] * 11
    assert set(mine) == set(theirs) and mine["square_avg"].shape == theirs["square_avg"].shape == (0,)


@pytest.mark.parametrize("family", ["plain", "warm"])
@pytest.mark.parametrize("max_norm", [0.0, -1.0])
def test_max_norm_zero_and_negative_are_pytorchs_formula(max_norm, family):
    """clip_grad_norm_(…, 0.0) zeroes the gradients and a negative max_norm turns them round: coef = max_norm / (norm + 1e-6),
    clamped from above alone.  Gradients, state and parameters against the fp64 evaluation of that formula."""
    from safe_marl_amd.optim import clip_and_step
    fam = fb.optim_case("actor")[family]
    opt, params, slabs = _setup(fam)
    snap, live = _snapshot(opt, params)
    yard, ref = _yardstick(snap, max_norm), _reference(snap, max_norm)
    norm = clip_and_step(opt, params, max_norm)
    th.cuda.synchronize()
    assert all(s.intact() for s in slabs)
    kern = {"norm": norm, "param": params, "grad": [p.grad for p in params], "square_avg": [opt.state[p]["square_avg"] for p in params]}
    fb.optim_within_budget(kern, yard, ref, name=f"optim actor {family} max_norm {max_norm}")
    sign = th.cat(kern["grad"]) * th.cat(snap[1])
    assert bool((sign == 0).all()) if max_norm == 0.0 else bool((sign <= 0).all() and (sign < 0).any())
    assert all(float(opt.state[p]["step"]) == 1.0 for p in params)


# ---------------------------------------------------------------------------------------------------------------------------
# the rider past the first trip

def test_the_refresh_rides_in_the_step_at_three_passes():
    """tests/test_optim_gpu.py's statement (flexnet_clip_rmsprop_refresh = the plain step + flexnet_window_refresh, bit for bit)
    at 140 017 elements in five tensors: the optimiser's blocks take three trips while the refresh's blocks ride behind them."""
    import ctypes as C
    from safe_marl_amd import _lib
    from safe_marl_amd.optim import clip_and_step
    from .test_optim_gpu import refresh_args
    lib = _lib.load()
    rows, n, act_w, stride, cap, start = 32768, 5, 20, 27, 200000, 200000 * 5 + 190000
    small = th.randn(cap, stride, device="cuda", generator=th.Generator(device="cuda").manual_seed(7))
    start_cell = th.tensor([start], dtype=th.int64, device="cuda")
    fam = fb.optim_case("three_passes")["warm"]
    res = []
    for ride in (True, False):
        opt, params, slabs = _setup(fam)
        ws = th.zeros(_lib.FLEXNET_TD_WS_FLOATS // 2, dtype=th.float64, device="cuda")
        refresh, out, cell = refresh_args(ws, small, start_cell, rows, n, act_w, stride, cap)
        noted = _fallbacks()
        if ride:
            norm = clip_and_step(opt, params, 1.0, refresh=refresh)
        else:
            norm = clip_and_step(opt, params, 1.0)
            _lib.check(lib.flexnet_window_refresh(C.byref(refresh[0]), C.byref(refresh[1]), C.c_void_p(th.cuda.current_stream().cuda_stream)),
                       "flexnet_window_refresh")
        th.cuda.synchronize()
        assert _fallbacks() == noted and all(s.intact() for s in slabs)
        res.append(({"norm": norm.clone(), "param": params, "grad": slabs[1].views, "square_avg": slabs[2].views,
                     "step": [opt.state[p]["step"] for p in params]}, out, cell.clone(), ws[:_lib.FLEXNET_TD_STAT_DOUBLES].clone()))
    (ka, oa, ca, wa), (kb, ob, cb, wb) = res
    _same_bits(ka, kb)
    idx = (start + th.arange(rows, device="cuda")) % cap
    for o in (oa, ob):
        assert th.equal(o["action"], small[idx, :act_w]) and th.equal(o["reward"], small[idx, act_w:act_w + n])
    assert ca.item() == cb.item() == start % cap
    assert th.equal(wa, wb) and bool(wa.abs().sum() > 0)


# ---------------------------------------------------------------------------------------------------------------------------
# util.mean_all

@pytest.mark.parametrize("kind", fb.MEAN_INPUTS)
@pytest.mark.parametrize("n", fb.MEAN_SIZES)
def test_mean_all_is_within_the_derived_bound(n, kind):
    """Both signs: the value through util.mean_all against ``fb.mean_within_bound``; the same bits from the entry point writing
    between sentinels, which keep theirs; the gradient under util.unit_seed and under an ordinary upstream gradient against
    ``x.mean()``'s, to one ulp."""
    from safe_marl_amd import _lib
    from safe_marl_amd.util import mean_all, unit_seed
    x_cpu = fb.mean_input(kind, n, th.Generator().manual_seed(100 * n + fb.MEAN_INPUTS.index(kind)))
    x = x_cpu.cuda()
    ws = th.zeros(_lib.FLEXNET_SUM_WS_FLOATS // 2, dtype=th.float64, device="cuda")
    up = th.tensor(0.37, device="cuda")
    for sign in (1.0, -1.0):
        out = mean_all(x, sign)
        assert out.dim() == 0 and out.dtype == th.float32
        fb.mean_within_bound(out, x_cpu, sign, name=f"mean_all {kind} n={n} sign={sign:+.0f}")
        slab = Slab([th.zeros(1)])
        a = _lib.FlexSumArgs()
        a.n, a.scale = n, sign / n
        a.x, a.out, a.workspace, a.workspace_floats = x.data_ptr(), slab.views[0].data_ptr(), ws.data_ptr(), 2 * ws.numel()
        _lib.launch("flexnet_scaled_sum", a)
        th.cuda.synchronize()
        assert slab.intact() and th.equal(slab.views[0].view(th.int32), out.reshape(1).view(th.int32))
        for seed in (unit_seed("cuda"), up):
            leaf, twin = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            (got,) = th.autograd.grad(mean_all(leaf, sign), leaf, grad_outputs=seed)
            (want,) = th.autograd.grad((twin if sign == 1.0 else -twin).mean(), twin, grad_outputs=seed.clone())
            assert got.shape == want.shape == x.shape
            assert bool(((got - want).abs() <= 2.0 ** -23 * want.abs()).all()), (n, kind, sign)
