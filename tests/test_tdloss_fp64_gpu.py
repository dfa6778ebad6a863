"""The stand-alone value loss of csrc/tdloss.hip (nets.td_loss) and its statistics-only pass
(nets.batchnorm_update_running_stats) on the fp64 error budget of tests/fp64_budget.py: loss, dq and the BatchNorm's running
statistics against ``fb.td_run`` in fp64 on the same fp32 numbers — at one row (no normalisation: a BatchNorm takes two), two
rows (unbiased factor 2), 4 099, 16 385 (one thread of the 64 x 256 takes a second row) and 65 537 rows (the second trip of
the statistics pass's four-deep loop), on tests/test_tdloss_gpu.py's rewards and on a column of failure rewards, where the
batch variance ss / rows - mean^2 of csrc/flex_td.h is a difference of numbers 1.6e7 times itself.  The figures of a run are
filed in profiles/fp64_error_budget.txt."""
import pytest
import torch as th

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

ROWS = (1, 2, 4099, 16385, 65537)
AGENTS = (1, 5, 8)


def td_case(rows, n, family):
    return fb.td_families(rows, n, th.Generator().manual_seed(1000 * rows + n))[family]


@pytest.mark.parametrize("family", fb.TD_FAMILIES)
@pytest.mark.parametrize("n", AGENTS)
@pytest.mark.parametrize("rows", ROWS)
def test_td_loss_and_the_statistics_only_pass(rows, n, family):
    from safe_marl_amd.nets import batchnorm_stats_supported, batchnorm_update_running_stats, td_loss, td_loss_supported
    fam = td_case(rows, n, family)
    norm = rows > 1
    make = lambda dtype, dev: fb.bn_module(n, dtype, dev, seed=3) if norm else None
    ref, t32 = fb.td_run(fam.inputs, fb.GAMMA, make(th.float64, "cpu"), th.float64), fb.td_run(fam.inputs, fb.GAMMA, make(th.float32, "cpu"), th.float32)
    q, nq, reward, done = (t.cuda() for t in fam.inputs)
    q = q.requires_grad_(True)
    bn = make(th.float32, "cuda")
    assert td_loss_supported(q, nq, reward, done, bn)
    loss = td_loss(q, nq, reward, done, fb.GAMMA, bn)
    (dq,) = th.autograd.grad(loss, [q])
    tag = f"td-loss {family} {rows}x{n}"
    fb.within_budget(loss.detach().cpu(), t32["loss"], ref["loss"], name=f"{tag} loss")
    fb.within_budget(dq.cpu(), t32["dq"], ref["dq"], name=f"{tag} dq")
    if not norm:
        return
    only = make(th.float32, "cuda")
    assert batchnorm_stats_supported(only, reward)
    batchnorm_update_running_stats(only, reward)
    for label, m in (("", bn), (" (statistics only)", only)):
        for stat in ("running_mean", "running_var"):
            fb.within_budget(getattr(m, stat).cpu(), t32[stat], ref[stat], name=f"{tag} {stat}{label}")
        assert int(m.num_batches_tracked) == int(ref["num_batches_tracked"]) == 1
    assert th.equal(bn.running_mean, only.running_mean) and th.equal(bn.running_var, only.running_var)


@pytest.mark.parametrize("rows", [2, 4099, 65537])
def test_failure_column_batch_statistics(rows):
    """The batch statistics of the failure family's reward columns, each column against ITSELF (a tensor-wide maximum would
    hide a column whose variance is 2.5e-3 behind one whose variance is 9): with momentum 1 the running statistics ARE the
    batch mean and the unbiased batch variance.  |mean| / std = 4 000 in column 1; column 0 is constant, its variance exactly
    zero in every form."""
    from safe_marl_amd.nets import batchnorm_update_running_stats
    n = 5
    reward = td_case(rows, n, "failure").inputs[2]
    forms = []
    for dtype, dev in ((th.float64, "cpu"), (th.float32, "cpu"), (th.float32, "cuda")):
        bn = fb.bn_module(n, dtype, dev, seed=3)
        bn.momentum = 1.0
        if dev == "cuda":
            batchnorm_update_running_stats(bn, reward.cuda())
        else:
            with th.no_grad():
                bn(reward.to(dtype))
        forms.append((bn.running_mean.cpu(), bn.running_var.cpu()))
    ref, t32, got = forms
    assert float(ref[1][0]) == 0.0 and float(got[1][0]) == 0.0 and float(got[0][0]) == fb.FAILURE_REWARD
    for j in range(n):
        for k, stat in enumerate(("mean", "var")):
            fb.within_budget(got[k][j:j + 1], t32[k][j:j + 1], ref[k][j:j + 1], name=f"td-stats failure {rows}x{n} batch {stat} of column {j}")
