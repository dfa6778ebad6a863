"""csrc/wgrad.hip (include/flexnet.h: flexnet_wgrad) — dW = dY^T X over a tall batch, the weight gradients that
loss.backward() forms in the reference's update (madrl/utils/trainer.py:62-111) for fc1 / GRUCell / fc2 of
rnn_agent.py:13-33 and fc1 of mlp_critic.py:5-34 — against an fp64 product of the same operands.  fp32 products and
sums: the tolerance is relative to the largest entry and grows with the square root of the batch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [
    (163840, 64, 149),      # actor fc1 at the update batch (32 768 samples x 5 agents)
    (163840, 192, 64),      # GRUCell weight_ih / weight_hh
    (163840, 4, 64),        # actor fc2
    (32768, 64, 720),       # critic fc1, observation columns (five column chunks)
    (32768, 64, 20),        # critic fc1, action columns
    (4099, 64, 149), (2051, 192, 33), (1000, 33, 161), (777, 100, 64), (64, 1, 1), (5, 3, 7), (1, 64, 64), (2, 192, 745),
]


def _ref(dy, x):
    return dy.double().t() @ x.double()


def _close(got, want, k):
    scale = max(want.abs().max().item(), 1e-30)
    return (got.double() - want).abs().max().item() / scale < 3e-7 * max(1.0, k ** 0.5)


def _colsum_in_budget(cs, dy, name):
    """The column sum under the fp64 error budget (tests/fp64_budget.py): three times the error of the library's fp32 sum plus
    FLOOR_ULPS and what a row-order running fp32 sum loses (``row_sum_rounding``)."""
    from . import fp64_budget as fb
    want = dy.double().sum(0)
    fb.within_budget(cs, dy.sum(0), want, floor_ulps=fb.floor_ulps(fb.row_sum_rounding(dy), want), name=name)


@pytest.mark.parametrize("k,m,n", SHAPES)
def test_matches_fp64_product(k, m, n):
    from safe_marl_amd.nets import tall_wgrad, tall_wgrad_supported
    g = torch.Generator(device="cuda").manual_seed(k + m + n)
    dy = torch.randn(k, m, device="cuda", generator=g)
    x = torch.randn(k, n, device="cuda", generator=g)
    assert tall_wgrad_supported(dy, x)
    got = tall_wgrad(dy, x)
    assert got.shape == (m, n)
    assert _close(got, _ref(dy, x), k)
    assert torch.equal(got, tall_wgrad(dy, x))                   # fixed summation order
    cs = torch.full((m,), float("nan"), device="cuda")
    again = tall_wgrad(dy, x, colsum=cs)                         # the bias gradient from the same pass
    assert torch.equal(again, got)
    want = dy.double().sum(0)
    assert (cs.double() - want).abs().max().item() <= 3e-7 * max(1.0, k ** 0.5) * max(dy.abs().max().item(), 1e-30) * max(1.0, k ** 0.5)
    _colsum_in_budget(cs, dy, f"wgrad {k}x{m}x{n} colsum")        # (the bound above allows 1e-4 of a column sum at 163 840 rows)


@pytest.mark.parametrize("k", [32768, 1003])
def test_row_strided_operands_are_read_in_place(k):
    """Column slices of wider records (the packed replay rows); neighbours hold NaN to prove nothing else is used."""
    from safe_marl_amd.nets import tall_wgrad, tall_wgrad_supported
    g = torch.Generator(device="cuda").manual_seed(7)
    rec_a = torch.full((k, 100), float("nan"), device="cuda")
    rec_b = torch.full((k, 400), float("nan"), device="cuda")
    dy, x = rec_a[:, 17:81], rec_b[:, 33:182]
    dy.copy_(torch.randn(k, 64, device="cuda", generator=g))
    x.copy_(torch.randn(k, 149, device="cuda", generator=g))
    assert tall_wgrad_supported(dy, x) and not x.is_contiguous()
    got = tall_wgrad(dy, x)
    assert torch.isfinite(got).all()
    assert _close(got, _ref(dy, x), k)


def test_accumulate_and_out():
    from safe_marl_amd.nets import tall_wgrad
    g = torch.Generator(device="cuda").manual_seed(3)
    dy = torch.randn(5000, 64, device="cuda", generator=g)
    x = torch.randn(5000, 70, device="cuda", generator=g)
    out = torch.ones(64, 70, device="cuda")
    same = tall_wgrad(dy, x, out=out, accumulate=True)
    assert same is out
    assert _close(out - 1.0, _ref(dy, x), 5000)


def test_tall_linear_gradients_match_the_library():
    """tall_linear is F.linear with the hand-written weight gradient."""
    from safe_marl_amd.nets import tall_linear
    import torch.nn.functional as F
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(20480, 64, device="cuda", generator=g)
    w = torch.randn(192, 64, device="cuda", generator=g) * 0.1
    b = torch.randn(192, device="cuda", generator=g)
    up = torch.randn(20480, 192, device="cuda", generator=g)
    outs = []
    for fn in (tall_linear, F.linear):
        xs, ws, bs = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = fn(xs, ws, bs)
        outs.append((y,) + torch.autograd.grad((y * up).sum(), [xs, ws, bs]))
    for a, e in zip(*outs):
        assert (a - e).abs().max().item() <= 2e-4 * max(1.0, e.abs().max().item())


def test_unsupported_shapes_are_refused():
    import ctypes as C
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import tall_wgrad_supported
    dy = torch.randn(100, 200, device="cuda")
    x = torch.randn(100, 8, device="cuda")
    assert not tall_wgrad_supported(dy, x)                        # m > 192
    assert not tall_wgrad_supported(dy[:, :64].t().t()[:, ::2], x)   # column stride 2
    lib = _lib.load()
    a = _lib.FlexWgradArgs()
    a.k, a.m, a.n, a.lda, a.ldb = 100, 200, 8, 200, 8
    out = torch.empty(200, 8, device="cuda")
    ws = torch.empty(_lib.FLEXNET_WGRAD_WS_FLOATS, device="cuda")
    a.a, a.b, a.c, a.workspace, a.workspace_floats = dy.data_ptr(), x.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel()
    assert lib.flexnet_wgrad(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.m, a.lda = 64, 32
    assert lib.flexnet_wgrad(C.byref(a), None) == -1      # FLEXNET_EINVAL


def test_actor_update_pass_matches_the_module_path():
    """RNNAgent.forward at an update batch (GRUCell composed from the gate GEMMs + ATen's fused cell, weight gradients
    from csrc/wgrad.hip) against the plain nn.GRUCell / nn.Linear path: same outputs, gradients to fp32 accuracy."""
    import types
    from safe_marl_amd import nets
    torch.manual_seed(0)
    args = types.SimpleNamespace(hid_size=64, layernorm=True, hid_activation="relu", action_dim=4, agent_num=5)
    agent = nets.RNNAgent(149, args).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = 20480
    obs = torch.randn(rows, 149, device="cuda", generator=g)
    hid = torch.randn(rows, 64, device="cuda", generator=g)
    up_a = torch.randn(rows, 4, device="cuda", generator=g)
    up_h = torch.randn(rows, 64, device="cuda", generator=g)
    params = list(agent.parameters())

    def run():
        h0 = hid.clone().requires_grad_(True)
        a, _, h = agent(obs, h0)
        return (a, h) + torch.autograd.grad((a * up_a).sum() + (h * up_h).sum(), [h0] + params)

    assert nets._FUSED_GRU is not None
    fast = run()
    saved, nets._FUSED_GRU, nets.WGRAD_MIN_ROWS = (nets._FUSED_GRU, nets.WGRAD_MIN_ROWS), None, 1 << 30
    try:
        plain = run()
    finally:
        nets._FUSED_GRU, nets.WGRAD_MIN_ROWS = saved
    for a, e in zip(fast, plain):     # outputs differ by the order in which the cell adds its biases (1 ulp)
        assert (a - e).abs().max().item() <= 1e-4 * max(1.0, e.abs().max().item())


@pytest.mark.parametrize("k,n,n2", [(32768, 720, 20), (4099, 720, 20), (2051, 150, 7), (1000, 160, 160), (515, 75, 161)])
def test_second_input_block_in_the_same_launch(k, n, n2):
    """[x | x2] read from their two homes as ONE operand (the critic's observation and action blocks, maddpg.py:47-54):
    the same numbers, bit for bit, as two separate calls; both blocks are column slices of wider records with NaN
    neighbours, and the outputs are column blocks of one wider gradient."""
    import ctypes as C
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import tall_wgrad
    g = torch.Generator(device="cuda").manual_seed(k + n + n2)
    dy = torch.randn(k, 64, device="cuda", generator=g)
    rec1 = torch.full((k, n + 9), float("nan"), device="cuda")
    rec2 = torch.full((k, n2 + 6), float("nan"), device="cuda")
    x, x2 = rec1[:, 4:4 + n], rec2[:, 3:3 + n2]
    x.copy_(torch.randn(k, n, device="cuda", generator=g))
    x2.copy_(torch.randn(k, n2, device="cuda", generator=g))
    dW = torch.full((64, n + 5 + n2), float("nan"), device="cuda")
    cs = torch.empty(64, device="cuda")
    tall_wgrad(dy, x, out=dW[:, :n], colsum=cs, x2=x2, out2=dW[:, n + 5:])
    assert torch.isnan(dW[:, n:n + 5]).all()                       # nothing written between the two blocks
    want1, want2 = tall_wgrad(dy, x), tall_wgrad(dy, x2)
    assert torch.equal(dW[:, :n], want1)
    assert _close(dW[:, n + 5:], _ref(dy, x2), k)
    if n2 <= 64 and n % 5 == 0:
        # the separate call sums the same products over the same row blocks only when both calls split the rows alike;
        # what must hold always is agreement within fp32 summation error and run-to-run reproducibility
        again = torch.empty_like(dW)
        tall_wgrad(dy, x, out=again[:, :n], x2=x2, out2=again[:, n + 5:])
        assert torch.equal(again[:, n + 5:], dW[:, n + 5:]) and torch.equal(again[:, :n], dW[:, :n])
    assert (want2 - dW[:, n + 5:]).abs().max().item() <= 3e-7 * k ** 0.5 * max(1.0, want2.abs().max().item())
    assert (cs.double() - dy.double().sum(0)).abs().max().item() <= 1e-3
    _colsum_in_budget(cs, dy, f"wgrad two blocks {k}x64x({n}|{n2}) colsum")
    # the entry point itself refuses what the kernel does not cover (the wrapper then makes two calls)
    lib = _lib.load()
    a = _lib.FlexWgradArgs()
    ws = torch.empty(_lib.FLEXNET_WGRAD_WS_FLOATS, device="cuda")
    out = torch.empty(64, 64, device="cuda")
    a.k, a.m, a.n, a.lda, a.ldb = 100, 64, 64, 64, 64
    a.a, a.b, a.c, a.workspace, a.workspace_floats = dy.data_ptr(), dy.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel()
    a.b2, a.c2, a.ldb2, a.n2 = dy.data_ptr(), out.data_ptr(), 64, 8
    assert lib.flexnet_wgrad(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED     # n <= 64: not the five-column lane shape
    a.n2 = 0
    assert lib.flexnet_wgrad(C.byref(a), None) == -1                            # b2 without columns
