"""The agent-summed action selection (matd3.py:88-111, iddpg.py:61-83) has ONE body in learner.py: MATD3's and IDDPG's
get_actions differ only in MATD3's masking of unavailable actions and its ``clip`` flag.  With every action available the two
return bit-equal tuples from the same policy weights and the same draws — what RolloutGraph.summed relies on when it replaces
either with one kernel; with an action unavailable MATD3 zeroes its mean and log-std and both zero the restored action."""
import pytest
import torch as th

from safe_marl_amd.learner import COMA, IDDPG, IPPO, MATD3, SQDDPG

from .golden_io import golden_args

ROWS = 7
MODES = [("train", True), ("train", False), ("test", False)]


def _pair(prefix, **over):
    """An IDDPG and a MATD3 with the same policy weights; the targets' policies differ from the behaviour policies."""
    args = golden_args(prefix, **over)
    th.manual_seed(0)
    iddpg, matd3 = IDDPG(args, IDDPG(args)), MATD3(args, MATD3(args))
    th.manual_seed(1)
    iddpg.target_net.policy_dicts.apply(iddpg.init_weights)
    matd3.policy_dicts.load_state_dict(iddpg.policy_dicts.state_dict())
    matd3.target_net.policy_dicts.load_state_dict(iddpg.target_net.policy_dicts.state_dict())
    g = th.Generator().manual_seed(2)
    obs = th.randn(ROWS, args.agent_num, args.obs_size, generator=g)
    hid = 0.1 * th.randn(ROWS, args.agent_num, args.hid_size, generator=g)
    return args, iddpg, matd3, obs, hid


def _flat(out):
    actions, restored, log_prob, (means, log_stds), hiddens = out
    return actions, restored, log_prob, means, log_stds, hiddens


def _call(model, obs, hid, status, explore, avail, target):
    th.manual_seed(3)
    return _flat(model.get_actions(obs, status=status, exploration=explore, actions_avail=avail, target=target, last_hid=hid))


@pytest.mark.parametrize("prefix", ["learner", "learner3"])
@pytest.mark.parametrize("enforcebound", [True, False])
def test_matd3_and_iddpg_select_the_same_actions_when_all_are_available(prefix, enforcebound):
    args, iddpg, matd3, obs, hid = _pair(prefix, action_enforcebound=enforcebound)
    for status, explore in MODES:
        for target in (False, True):
            for const in (False, True):
                avail = th.ones(ROWS, args.agent_num, args.action_dim)
                if const:
                    avail._flex_const = 1.0
                a = _call(iddpg, obs, hid, status, explore, avail, target)
                b = _call(matd3, obs, hid, status, explore, avail, target)
                for i, (x, y) in enumerate(zip(a, b)):
                    assert (x is None and y is None) or th.equal(x, y), (status, explore, target, const, i)
                assert a[1].shape == (ROWS, args.agent_num, args.action_dim)


@pytest.mark.parametrize("prefix", ["learner", "learner3"])
def test_an_unavailable_action_is_masked_by_matd3_and_restored_to_zero_by_both(prefix):
    args, iddpg, matd3, obs, hid = _pair(prefix, fixed_policy_std=0.5)          # (log-std = log 0.5: not zero by itself)
    avail = th.ones(ROWS, args.agent_num, args.action_dim)
    avail[:, 1, 2] = 0.0
    for status, explore in MODES:
        a = _call(iddpg, obs, hid, status, explore, avail, False)
        b = _call(matd3, obs, hid, status, explore, avail, False)
        for k in (3, 4):                       # means, log-stds
            assert th.count_nonzero(b[k][:, 1, 2]) == 0 and th.count_nonzero(a[k][:, 1, 2]) == ROWS
            assert th.count_nonzero(b[k]) == b[k].numel() - ROWS
        for out in (a, b):                     # the restored actions: zero there and nowhere else
            assert th.count_nonzero(out[1][:, 1, 2]) == 0 and th.count_nonzero(out[1]) == out[1].numel() - ROWS


def test_which_classes_share_which_method():
    assert SQDDPG.get_actions is IDDPG.get_actions
    assert IPPO.get_actions is IDDPG.get_actions
    assert COMA.get_actions is IDDPG.get_actions
    assert MATD3.get_actions is not IDDPG.get_actions
