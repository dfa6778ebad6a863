"""The outputs of the four per-agent critic entry points (csrc/critic_unshared.hip, csrc/critic_unshared_twin.hip) of one source
tree on fixed inputs, for a bit-for-bit comparison of two trees — a refactor's parent and its branch:

    python tools/critic_unshared_bits.py dump --root TREE OUT.pt      (once per tree, each in a process of its own)
    python tools/critic_unshared_bits.py compare A.pt B.pt

``dump`` imports the package of ``TREE`` (default: this one), whose library must be built, and calls the entry points
directly.  Inputs and weights come from a CPU generator seeded per case.  Shapes: the CASES of
tests/test_critic_unshared_gpu.py (its four input forms) for the plain family and of tests/test_critic_unshared_twin_gpu.py
for the twins (one and two heads), and for both the two shapes past 16 384 samples per agent, where a backward wavefront
walks a second tile.  Every case runs the forward with and without the saves and the backward with and without
``param_grads``, with and without ``d_x2_own``.  Every output buffer is pre-filled with a sentinel, so the elements a
launch leaves alone are compared too.  ``compare`` applies torch.equal to every tensor and prints one line per kernel family
and output; its exit status is 1 unless everything is identical."""
import argparse
import os
import sys

import torch as th

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0
SEVERAL_TILES = [(16417, 1, True), (16385, 2, False)]        # (b, n, layernorm) of test_a_wavefront_that_walks_several_tiles
SUMS = ("d_ln_w", "d_ln_b", "d_fc1_b", "d_fc2_b", "d_fc3_w")


def cases():
    """(family, b, n, shared, has_act, obs_dim, act_dim, layernorm, agent_id, heads)"""
    sys.path.insert(0, HERE)
    from tests.test_critic_unshared_gpu import CASES as PLAIN, FORMS
    from tests.test_critic_unshared_twin_gpu import CASES as TWIN
    out = [("plain", b, n, *FORMS[form], o, a, ln, aid, None) for b, n, form, o, a, ln, aid in PLAIN]
    out += [("plain", b, n, True, True, 6, 2, ln, True, None) for b, n, ln in SEVERAL_TILES]
    for heads in (1, 2):
        out += [("twin", b, n, True, True, o, a, ln, aid, heads) for b, n, o, a, ln, aid in TWIN]
        out += [("twin", b, n, True, True, 6, 2, ln, True, heads) for b, n, ln in SEVERAL_TILES]
    return out


def filled(*shape):
    return th.full(shape, SENTINEL, dtype=th.float32, device="cuda")


def run_case(_lib, case):
    family, b, n, shared, has_act, o, a, ln, aid, heads = case
    twin = family == "twin"
    hd = heads or 1
    gen = th.Generator().manual_seed(1000 * b + 10 * n + hd)

    def rand(*shape, scale=1.0):
        return (scale * th.randn(*shape, generator=gen)).cuda()

    w1, w2 = o * (n if shared else 1), (a * (n if shared else 1)) if has_act else 0
    ld = w1 + (n if aid else 0) + w2 + (1 if twin else 0)
    weights = [dict(fc1_w=rand(64, ld, scale=0.2), fc1_b=rand(64, scale=0.2), ln_w=1.0 + rand(64, scale=0.2), ln_b=rand(64, scale=0.2),
                    fc2_w=rand(64, 64, scale=0.2), fc2_b=rand(64, scale=0.2), fc3_w=rand(1, 64, scale=0.2), fc3_b=rand(1, scale=0.2))
               for _ in range(n)]
    obs, act, dq = rand(b, n, o, scale=0.5), rand(b, n, a, scale=0.5), rand(hd, b, n) / (b * n)
    rows = b * n
    fwd_cls, bwd_cls = ((_lib.FlexCriticUnsharedTwinArgs, _lib.FlexCriticUnsharedTwinBwdArgs) if twin else
                        (_lib.FlexCriticUnsharedArgs, _lib.FlexCriticUnsharedBwdArgs))
    stem = "flexnet_critic_unshared_twin" if twin else "flexnet_critic_unshared"

    def head(s):
        s.rows, s.n_agents, s.w1, s.w2, s.agent_id, s.layernorm, s.ln_eps = rows, n, w1, w2, int(aid), int(ln), 1e-5
        if twin:
            s.heads = heads
        names = {f[0] for f in s._fields_}
        for i, w in enumerate(weights):
            for k, t in w.items():
                if k in names and (ln or not k.startswith("ln_")):
                    getattr(s, k)[i] = t.data_ptr()
        return s

    out = {}
    saves = None
    for save in (True, False):
        f = head(fwd_cls())
        f.x1, f.x1_pitch, f.x1_agent_off = obs.data_ptr(), n * o, 0 if shared else o
        if has_act:
            f.x2, f.x2_pitch, f.x2_agent_off = act.data_ptr(), n * a, 0 if shared else a
        bufs = {"q": filled(hd, b, n)}
        if save:
            bufs.update(save_z1=filled(rows, 64), save_x=filled(hd, rows, 64))
            saves = bufs
        for k, t in bufs.items():
            setattr(f, k, t.data_ptr())
        _lib.launch(stem + "_forward", f)
        out.update({f"forward saves {save} {k}": t for k, t in bufs.items()})
    for pg in (True, False):
        for own in ((True, False) if has_act else (False,)):
            g = head(bwd_cls())
            g.param_grads = int(pg)
            g.dq, g.z1, g.x = dq.data_ptr(), saves["save_z1"].data_ptr(), saves["save_x"].data_ptr()
            bufs = {"dz1_sum" if twin else "dz1": filled(rows, 64), "dz2": filled(hd, rows, 64), "d_fc3_b": filled(n)}
            bufs.update({k: filled(n, 64) for k in SUMS + (("d_flag",) if twin else ())})
            for k, t in bufs.items():
                setattr(g, k, t.data_ptr())
            bufs["d_x2_own"] = filled(rows, a)
            if own:
                g.d_x2_own, g.own_first, g.own_step, g.own_w = bufs["d_x2_own"].data_ptr(), 0, a if shared else 0, a
            ws = filled(_lib.FLEXNET_CRITIC_UNSHARED_TWIN_WS_FLOATS if twin else _lib.FLEXNET_CRITIC_UNSHARED_WS_FLOATS)
            g.workspace, g.workspace_floats = ws.data_ptr(), ws.numel()
            _lib.launch(stem + "_backward", g)
            out.update({f"backward param_grads {pg} own {own} {k}": t for k, t in bufs.items()})
    th.cuda.synchronize()
    return {k: t.cpu() for k, t in out.items()}


def dump(root, path):
    sys.path.insert(0, root)
    import safe_marl_amd  # noqa: F401
    from safe_marl_amd import _lib, build
    assert os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))) == os.path.abspath(root), _lib.__file__
    assert build.built_digest() == build.source_digest(), "the tree's library is not built from its sources"
    res = {"digest": build.source_digest(), "cases": {}}
    for case in cases():
        res["cases"][" ".join(str(c) for c in case)] = run_case(_lib, case)
    th.save(res, path)
    print(f"{root}: library {res['digest'][:16]}, {len(res['cases'])} cases, "
          f"{sum(len(v) for v in res['cases'].values())} tensors -> {path}")


def compare(path_a, path_b):
    a, b = th.load(path_a), th.load(path_b)
    print(f"A: library {a['digest'][:16]}    B: library {b['digest'][:16]}")
    assert sorted(a["cases"]) == sorted(b["cases"])
    tally, differ = {}, []
    for case, ta in a["cases"].items():
        tb = b["cases"][case]
        assert sorted(ta) == sorted(tb), case
        for k, t in ta.items():
            words = k.split()
            key = (case.split()[0], words[0], words[-1])
            same = t.shape == tb[k].shape and th.equal(t, tb[k])
            n, bad, untouched = tally.get(key, (0, 0, 0))
            tally[key] = (n + 1, bad + (not same), untouched + bool((t == SENTINEL).all()))
            if not same:
                differ.append((case, k))
    print("family | launch   | output    | tensors compared | of them left at the sentinel by both | outcome")
    for (family, launch, name), (n, bad, untouched) in sorted(tally.items()):
        print(f"{family:6s} | {launch:8s} | {name:9s} | {n:4d} | {untouched:4d} | {'identical' if not bad else f'{bad} DIFFER'}")
    for case, k in differ[:40]:
        print("DIFFERS:", case, "|", k)
    print("outcome:", "identical everywhere" if not differ else f"{len(differ)} tensors differ")
    return 1 if differ else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("--root", default=HERE)
    d.add_argument("out")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    ns = ap.parse_args()
    if ns.cmd == "dump":
        dump(os.path.abspath(ns.root), ns.out)
    else:
        sys.exit(compare(ns.a, ns.b))
