"""csrc/qmix.hip (flexnet_qmix_forward / flexnet_qmix_backward + the flexnet_wgrad reductions) against fp32 PyTorch autograd
of the same QMixer (its reference composition, ``forward_torch``).  The fp64 error budget on edge-case inputs and shapes, the
bit-for-bit structure and the NaN rule are tests/test_qmix_fp64_gpu.py's."""
import warnings

import pytest
import torch as th

pytestmark = pytest.mark.gpu


def _args(n, obs=144):
    from safe_marl_amd.util import convert
    return convert(dict(agent_num=n, obs_size=obs, mixing_embed_dim=64, hypernet_layers=2, hypernet_embed=64,
                        hyper_initialization_nonzeros=0, gated=False, skip_connections=False))


def _mixer(n, seed=0, zero_rows=False):
    from safe_marl_amd.nets import QMixer
    th.manual_seed(seed)
    m = QMixer(_args(n)).cuda()
    with th.no_grad():
        for p in m.parameters():
            p.normal_(0.0, 0.1)
        if zero_rows:            # exact zeros in the hypernetworks' outputs: abs' sign(0) = 0 must come through
            m.hyper_w_1[2].weight[::7].zero_()
            m.hyper_w_1[2].bias[::7].zero_()
            m.hyper_w_final[2].weight[::5].zero_()
            m.hyper_w_final[2].bias[::5].zero_()
    return m


def _inputs(B, n, seed=1):
    g = th.Generator(device="cuda").manual_seed(seed)
    q = th.randn(B, n, device="cuda", generator=g)
    x = 0.3 * th.randn(B, n * 144, device="cuda", generator=g)
    w = th.randn(B, device="cuda", generator=g) / B
    return q, x, w


def _clear_ties(m, x, w, eps=1e-5):
    """Zero the loss weight of samples with a ReLU pre-activation or a hypernetwork output (before abs) within eps of 0
    (exact zeros excepted: both forms produce those exactly).  There the two fp32 forms may take different sides of the
    kink, a jump of one sample's whole contribution in a batch-summed gradient, whichever form is the more accurate."""
    import copy
    md = copy.deepcopy(m).double()
    X = x.double()
    with th.no_grad():
        tie = th.zeros(X.shape[0], dtype=th.bool, device=X.device)
        for head in (md.hyper_w_1, md.hyper_w_final, md.V):
            pre = head[0](X)
            tie |= ((pre.abs() < eps) & (pre != 0)).any(1)
            if head is not md.V:
                out = head[2](th.relu(pre))
                tie |= ((out.abs() < eps) & (out != 0)).any(1)
    w = w.clone()
    w[tie] = 0.0
    return w


def _run(m, q, x, w, fused):
    q = q.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    y = m(q, x) if fused else m.forward_torch(q, x)
    (y.view(-1) * w).sum().backward()
    return y.detach().view(-1), q.grad.clone(), {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("B,n,zero", [(32768, 5, False), (1000, 5, True), (4096, 3, False), (77, 3, True)])
def test_kernel_matches_autograd(B, n, zero):
    m = _mixer(n, zero_rows=zero)
    q, x, w = _inputs(B, n)
    w = _clear_ties(m, x, w)
    assert m.fused_supported(q, x)
    y, dq, grads = _run(m, q, x, w, True)
    y0, dq0, grads0 = _run(m, q, x, w, False)
    assert th.allclose(y, y0, atol=1e-4, rtol=1e-4), (y - y0).abs().max()
    assert th.allclose(dq, dq0, atol=1e-5 * max(1.0, float(dq0.abs().max())), rtol=1e-4), (dq - dq0).abs().max()
    # parameter gradients are sums over the whole batch with heavy cancellation: both fp32 forms are held against an fp64
    # evaluation of the same module, and the kernel's error may not exceed a few times the PyTorch composition's own
    m64 = _mixer(n, zero_rows=zero).double()
    _, _, grads64 = _run(m64, q.double(), x.double(), w.double(), False)
    for k, g64 in grads64.items():
        scale = max(1e-6, float(g64.abs().max()))
        err_k = float((grads[k].double() - g64).abs().max())
        err_t = float((grads0[k].double() - g64).abs().max())
        assert err_k <= 3.0 * err_t + 2e-4 * scale, (k, err_k, err_t, scale)


def test_value_step_form_skips_parameter_gradients_and_is_bit_identical_run_to_run():
    m = _mixer(5, seed=3)
    q, x, w = _inputs(8192, 5, seed=4)
    outs = []
    for _ in range(2):
        outs.append(_run(m, q, x, w, True))
    y1, dq1, g1 = outs[0]
    y2, dq2, g2 = outs[1]
    assert th.equal(y1, y2) and th.equal(dq1, dq2)
    assert all(th.equal(g1[k], g2[k]) for k in g1)
    qq = q.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    y = m(qq, x, param_grads=False)
    (y.view(-1) * w).sum().backward()
    assert all(p.grad is None for p in m.parameters())
    assert th.equal(qq.grad, dq1)


def test_unsupported_configuration_falls_back_to_the_composition():
    from safe_marl_amd.nets import QMixer
    a = _args(5)._replace(gated=True)
    m = QMixer(a).cuda()
    q, x, _ = _inputs(64, 5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert not m.fused_supported(q, x)
    y = m(q, x)
    assert th.allclose(y, m.forward_torch(q, x))
