"""The floors of the vector-sum gradients in tests/test_sqddpg_unshared_gpu.py: fb.tail_sum_floors's addends under
fb.ordered_sum_rounding instead of fb.row_sum_rounding.

tests/test_sqddpg_fp64_gpu.py holds the shared kernel's tail sums to fb.tail_sum_floors, whose fb.row_sum_rounding takes the
summed rows to be exchangeable.  The rows ONE agent's wavefront sums are not: it takes them sample by sample ((sample, s) order
within a chunk), and the ns rows of a sample carry the same d_phi[b, i] / ns and the same observations — for fc3.bias, with
only phi upstream, the very same addend ns times.  A cancelling sum of b values each repeated ns times has partial sums
sqrt(ns) times those of b ns shuffled values, and a running fp32 sum rounds in proportion to its partial sums.  (In the shared
kernel a tile's rows interleave the agents.)  Held to fb.tail_sum_floors as it stands, two gradients missed the bound
3 err(fp32 composition) + 8 ulps + row_sum_rounding:
  n = 3, a = 1, ns = 3, b = 64, no LayerNorm, no d_q: d_fc3.bias of critic 2 off by 9.8e-8 on a gradient of 1.8e-3 (about 900
  of its ulps; the partial sums reach 0.1, where 9.8e-8 is 16 ulps) against 6.9e-8;
  n = 5, a = 1, ns = 10, b = 26, LayerNorm, d_q given: d_fc2.bias of critic 0 off by 1.7e-7 on a largest entry of 7.8e-2 (37 of
  its ulps) against 1.33e-7.
``ordered_floor`` is fb.ordered_sum_rounding with one run per sample: what a running fp32 sum in this order does, which
fp64_budget names the least accurate order a correct kernel may use.  Margin and the 8-ulp floor stay fp64_budget's; fc1.bias
and every other gradient take no floor beyond them, as in the shared kernel's test."""
import torch as th

from . import fp64_budget as fb


def ordered_floor(addends, ns):
    """fb.ordered_sum_rounding of ``addends`` [b ns, ...] in (sample, s) order, the ns rows of a sample (exchangeable among
    themselves: coalitions of one draw) as one run that starts at the prefix P_j, the sum of the samples before it.  Written
    with cumulative sums instead of fb.ordered_sum_rounding's loop over runs (16 385 of them in the largest case);
    tests/test_sqddpg_unshared_cpu.py holds the two forms equal.  A wavefront's running sum covers only its own chunks and the
    wavefronts' sums are folded afterwards: one running sum over all of an agent's rows is the least accurate order the work
    map allows, so this figure bounds the kernel's from above."""
    a = addends.detach().double()
    a = a.view(a.shape[0] // ns, ns, *a.shape[1:])
    L = float(ns)
    m, v = a.mean(1), a.var(1, unbiased=False)
    p = th.cumsum(L * m, 0) - L * m                                            # the prefix before each run
    total = (L * p.square() + p * m * L ** 2 + m.square() * L ** 3 / 3.0 + v * L ** 2 / 6.0).sum(0)
    return 3.0 * fb.ULP * (total / 3.0).sqrt()


def vector_sum_floors(g_q, g_pre1, g_pre2, pre1, pre2, ln, ns):
    """fb.tail_sum_floors's addends, each under ``ordered_floor``: {parameter name: floor, shaped as the parameter}."""
    out = {"fc3.bias": ordered_floor(g_q, ns).reshape(1), "fc3.weight": ordered_floor(g_q * th.relu(pre2), ns).reshape(1, 64),
           "fc2.bias": ordered_floor(g_pre2, ns)}
    if ln is not None:
        out["layernorm.bias"] = ordered_floor(g_pre1, ns)
        out["layernorm.weight"] = ordered_floor(g_pre1 * (pre1 - ln.bias) / ln.weight, ns)
    return out
