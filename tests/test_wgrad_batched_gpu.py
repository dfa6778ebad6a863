"""csrc/wgrad.hip, flexnet_wgrad_batched (include/flexnet.h): independent weight gradients C_i = A_i^T B_i in one call — the
per-agent gradients of ``shared_params: False`` — against fp64 products of the same operands with tests/test_wgrad_gpu.py's
tolerance, and against flexnet_wgrad bit for bit where there is one problem."""
import ctypes as C

import pytest
import torch

from .test_wgrad_gpu import _close, _colsum_in_budget, _ref

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
GUARD = 3


def _guarded(rows, width):
    buf = torch.full((rows + 2 * GUARD, width), SENTINEL, device="cuda")
    return buf, buf[GUARD:GUARD + rows]


def _guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def _problem(a, dy, x, out, ws, colsum=None, accumulate=False):
    a.k, a.m, a.n = dy.shape[0], dy.shape[1], x.shape[1]
    a.lda, a.ldb = (dy.stride(0), x.stride(0)) if dy.shape[0] > 1 else (a.m, a.n)
    a.a, a.b, a.c, a.ldc = dy.data_ptr(), x.data_ptr(), out.data_ptr(), out.stride(0) if a.m > 1 else a.n
    a.workspace, a.workspace_floats, a.accumulate = ws.data_ptr(), ws.numel(), int(accumulate)
    a.colsum = None if colsum is None else colsum.data_ptr()


@pytest.mark.parametrize("k,m,n", [(4099, 64, 149), (2051, 192, 33), (1000, 33, 161), (5, 3, 7), (1, 64, 64), (2049, 64, 720)])
def test_one_problem_gives_the_bits_of_flexnet_wgrad(k, m, n):
    from safe_marl_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(k + m + n)
    dy = torch.randn(k, m, device="cuda", generator=g)
    x = torch.randn(k, n, device="cuda", generator=g)
    ws = torch.empty(_lib.FLEXNET_WGRAD_WS_FLOATS, device="cuda")
    outs = []
    for name in ("flexnet_wgrad", "flexnet_wgrad_batched"):
        out, cs = _guarded(m, n), _guarded(1, m)
        table = (_lib.FlexWgradArgs * 1)()
        _problem(table[0], dy, x, out[1], ws, colsum=cs[1])
        if name == "flexnet_wgrad":
            _lib.launch(name, table[0])
        else:
            _lib.launch(name, table, 1)
        torch.cuda.synchronize()
        assert _guards_untouched(out[0]) and _guards_untouched(cs[0])
        outs.append((out[0], cs[0]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert _close(outs[1][0][GUARD:GUARD + m], _ref(dy, x), k)


def _mixed_batch():
    """Three shape classes ([2, 5], [6, 2], [1, 1]); k among 1, 7, 64, 65 and 2 049; agent rows of interleaved [b, n, .]
    tensors through lda = 64 n; column-slice outputs; column sums; one accumulating problem."""
    g = torch.Generator(device="cuda").manual_seed(5)
    n_ag, b = 3, 2049
    dz = torch.randn(b, n_ag, 64, device="cuda", generator=g)
    obs = torch.randn(b, n_ag, 149, device="cuda", generator=g)
    wide = _guarded(n_ag * 64, 149 + n_ag + 7)                          # [n, 64, 159]: the x block of every agent's fc1 gradient
    d_fc1 = wide[1].view(n_ag, 64, 159)
    problems, bufs = [], [wide[0]]
    for i in range(n_ag):                                              # class [2, 5], k = 2 049, lda = 64 n, ldc = 159
        cs = _guarded(1, 64)
        bufs.append(cs[0])
        problems.append(dict(dy=dz[:, i], x=obs[:, i], out=d_fc1[i, :, :149], colsum=cs[1][0], accumulate=False))
    for k in (1, 7, 64, 65):                                           # class [6, 2] (GRUCell) and class [1, 1] (fc2), unequal k
        dy = torch.randn(k, 192, device="cuda", generator=g)
        x = torch.randn(k, 64, device="cuda", generator=g)
        out, cs = _guarded(192, 64), _guarded(1, 192)
        bufs += [out[0], cs[0]]
        problems.append(dict(dy=dy, x=x, out=out[1], colsum=cs[1][0] if k != 7 else None, accumulate=False))
        dy = torch.randn(k, 4, device="cuda", generator=g)
        out = _guarded(4, 30)
        bufs.append(out[0])
        acc = k == 65
        if acc:
            out[1].fill_(1.0)
        problems.append(dict(dy=dy, x=torch.randn(k, 30, device="cuda", generator=g), out=out[1], colsum=None, accumulate=acc))
    return problems, bufs, d_fc1


def _run(problems, ws):
    from safe_marl_amd import _lib
    table = (_lib.FlexWgradArgs * len(problems))()
    slice_floats = ws.numel() // len(problems)
    for i, (a, p) in enumerate(zip(table, problems)):
        _problem(a, p["dy"], p["x"], p["out"], ws[i * slice_floats:(i + 1) * slice_floats], p["colsum"], p["accumulate"])
    _lib.launch("flexnet_wgrad_batched", table, len(problems))
    torch.cuda.synchronize()
    return table


def test_a_mixed_batch_against_fp64_products():
    from safe_marl_amd import _lib
    problems, bufs, d_fc1 = _mixed_batch()
    assert len(problems) == 11
    ws = torch.empty(11 * (_lib.FLEXNET_WGRAD_CS_FLOATS + 8 * 12288), device="cuda")
    _run(problems, ws)
    for buf in bufs:
        assert _guards_untouched(buf)
    assert bool((d_fc1[:, :, 149:] == SENTINEL).all())                 # nothing written beside the column blocks
    for p in problems:
        k = p["dy"].shape[0]
        want = _ref(p["dy"], p["x"])
        got = p["out"] - 1.0 if p["accumulate"] else p["out"]
        assert _close(got, want, k), (k, p["out"].shape)
        if p["colsum"] is not None:
            cs = p["dy"].double().sum(0)
            assert (p["colsum"].double() - cs).abs().max().item() <= 3e-7 * max(1.0, k) * max(p["dy"].abs().max().item(), 1e-30)
            _colsum_in_budget(p["colsum"], p["dy"], f"wgrad batched {k}x{p['dy'].shape[1]} colsum")
    first = [b.clone() for b in bufs]
    for p in problems:                                                 # the accumulating problem starts from the same values
        if p["accumulate"]:
            p["out"].fill_(1.0)
    _run(problems, ws)
    for b0, b1 in zip(first, bufs):
        assert torch.equal(b0, b1)                                     # fixed summation order: the same bits


def test_the_wrapper_slices_its_own_workspace():
    """nets.tall_wgrad_batched on a node's problems: the values of per-problem tall_wgrad calls (another split of the rows, so
    fp32 summation error apart), the same bits twice."""
    from safe_marl_amd.nets import tall_wgrad, tall_wgrad_batched
    g = torch.Generator(device="cuda").manual_seed(9)
    n, b = 5, 4096
    dz = torch.randn(b, n, 64, device="cuda", generator=g)
    dgi = torch.randn(b, n, 192, device="cuda", generator=g)
    obs = torch.randn(b, n * 144, device="cuda", generator=g)
    x = torch.randn(b, n, 64, device="cuda", generator=g)
    d1 = torch.zeros(2, n, 64, n * 144 + n, device="cuda")
    d2 = torch.empty(2, n, 192, 64, device="cuda")
    db = torch.empty(2, n, 192, device="cuda")
    for rep in range(2):
        problems = []
        for i in range(n):
            problems += [(dz[:, i], obs, d1[rep, i, :, :n * 144], None), (dgi[:, i], x[:, i], d2[rep, i], db[rep, i])]
        tall_wgrad_batched(problems)
    assert torch.equal(d1[0], d1[1]) and torch.equal(d2[0], d2[1]) and torch.equal(db[0], db[1])
    assert bool((d1[0][:, :, n * 144:] == 0).all())
    for i in range(n):
        assert _close(d1[0, i, :, :n * 144], _ref(dz[:, i], obs), b)
        assert _close(d2[0, i], _ref(dgi[:, i], x[:, i]), b)
        single = tall_wgrad(dgi[:, i], x[:, i])
        assert (single - d2[0, i]).abs().max().item() <= 3e-7 * b ** 0.5 * max(1.0, single.abs().max().item())


def test_refusals_write_nothing():
    from safe_marl_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(2)
    dy = torch.randn(100, 64, device="cuda", generator=g)
    x = torch.randn(100, 64, device="cuda", generator=g)
    outs = [_guarded(64, 64) for _ in range(2)]
    ws = torch.full((2 * (_lib.FLEXNET_WGRAD_CS_FLOATS + 4096),), SENTINEL, device="cuda")
    half = ws.numel() // 2
    table = (_lib.FlexWgradArgs * 2)()
    _problem(table[0], dy, x, outs[0][1], ws[:half])
    _problem(table[1], dy, x, outs[1][1], ws[half - 1:2 * half - 1])                  # one float into the first slice
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.flexnet_wgrad_batched(table, 2, stream) == -1                          # FLEXNET_EINVAL
    _problem(table[1], dy, x, outs[1][1], ws[half:])
    table[1].b2, table[1].c2, table[1].ldb2, table[1].n2 = x.data_ptr(), outs[1][1].data_ptr(), 64, 8
    assert lib.flexnet_wgrad_batched(table, 2, stream) == _lib.FLEXNET_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((ws == SENTINEL).all()) and all(bool((o[0] == SENTINEL).all()) for o in outs)
    table[1].b2, table[1].c2, table[1].ldb2, table[1].n2 = None, None, 0, 0
    assert lib.flexnet_wgrad_batched(table, 2, stream) == 0                           # ... and the same table without it runs
    torch.cuda.synchronize()
    assert torch.equal(outs[0][1], outs[1][1]) and _close(outs[0][1], _ref(dy, x), 100)
