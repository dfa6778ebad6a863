"""csrc/wgrad.hip with csrc/wgrad_block.h (flexnet_wgrad, flexnet_wgrad_batched) under the fp64 error budget of
tests/fp64_budget.py: dW = dy^T x and the column sum of dy against the fp64 product of the same operands, the
yardstick the library's fp32 GEMM and sum on the GPU, the floor ``fb.wgrad_floors`` (what a row-order running fp32 sum loses;
tests/test_fp64_budget_cpu.py holds it on the very cases, drawn from a CPU generator).  Two shapes per shape class (MT, NT) on both
sides of every class boundary, seven input families, every output between sentinel guard rows; then the paths no earlier test
reads the numbers of: row-strided A below its tile width, ``b_row_cell``, ``accumulate`` on the column sum, the slab cap with a
ragged last slab, non-finite values that must stay in their row or column, a 16-problem table, the second input block."""
import pytest
import torch

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
GUARD = 3
_WS = {}


def _ws():
    from safe_marl_amd import _lib
    if "ws" not in _WS:
        _WS["ws"] = torch.empty(_lib.FLEXNET_WGRAD_WS_FLOATS, device="cuda")
    return _WS["ws"]


def _guarded(rows, width, fill=SENTINEL):
    buf = torch.full((rows + 2 * GUARD, width), SENTINEL, device="cuda")
    buf[GUARD:GUARD + rows] = fill
    return buf, buf[GUARD:GUARD + rows]


def _guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def _problem(a, dy, x, out, ws, colsum=None, accumulate=False):
    a.k, a.m, a.n = dy.shape[0], dy.shape[1], x.shape[1]
    a.lda, a.ldb = (dy.stride(0), x.stride(0)) if dy.shape[0] > 1 else (a.m, a.n)
    a.a, a.b, a.c, a.ldc = dy.data_ptr(), x.data_ptr(), out.data_ptr(), out.stride(0) if a.m > 1 else a.n
    a.workspace, a.workspace_floats, a.accumulate = ws.data_ptr(), ws.numel(), int(accumulate)
    a.colsum = None if colsum is None else colsum.data_ptr()


def _split(k, m, n, ws_floats, launch_chunks=None):
    """(slabs, rows per block) of csrc/wgrad.hip's wgrad_prepare: a function of k, the shape class and the workspace alone —
    the row pitches play no part, so a strided call and the call on contiguous copies split the rows alike."""
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import _wgrad_class
    _, _, chunks, img = _wgrad_class(m, n)
    slabs = min((k + 63) // 64, max(512 // (launch_chunks or chunks), 1), (ws_floats - _lib.FLEXNET_WGRAD_CS_FLOATS) // (chunks * img), 520)
    slabs = max(slabs, 1)
    rpb = max(((k + slabs - 1) // slabs + 7) & ~7, 8)
    return (k + rpb - 1) // rpb if k > 0 else 1, rpb


def _call(dy, x, colsum=True, accumulate=False, prefill=(SENTINEL, SENTINEL), cell=None, b_base=None):
    """One flexnet_wgrad launch into guarded outputs: (dW [m, n], column sum [m] or None), copies."""
    from safe_marl_amd import _lib
    k, m, n = dy.shape[0], dy.shape[1], x.shape[1]
    out, cs = _guarded(m, n, prefill[0]), _guarded(1, m, prefill[1])
    a = _lib.FlexWgradArgs()
    _problem(a, dy, x, out[1], _ws(), colsum=cs[1] if colsum else None, accumulate=accumulate)
    if cell is not None:
        a.b, a.b_row_cell = b_base.data_ptr(), cell.data_ptr()
    _lib.launch("flexnet_wgrad", a)
    torch.cuda.synchronize()
    assert _guards_untouched(out[0]) and _guards_untouched(cs[0]), (k, m, n)
    if not colsum:
        assert bool((cs[0] == SENTINEL).all())
    return out[1].clone(), cs[1][0].clone() if colsum else None


def _cuda(fam):
    return fb.Family(fam.name, tuple(t.cuda() for t in fam.inputs), fam.params, fam.groups)


def _held(got_c, got_cs, fam, tag):
    """dW and the column sum of one family (CUDA inputs) inside the budget; the yardstick is the library's fp32 GEMM."""
    dy, x = fam.inputs
    ref_c, ref_cs = fb.wgrad_plain(dy.double(), x.double())
    yard_c, yard_cs = fb.wgrad_plain(dy, x)
    floor_c, floor_cs = fb.wgrad_floors(fam)
    fb.within_budget(got_c, yard_c, ref_c, floor_ulps=fb.floor_ulps(floor_c, ref_c), name=f"wgrad {tag} {fam.name} dW")
    if got_cs is not None:
        fb.within_budget(got_cs, yard_cs, ref_cs, floor_ulps=fb.floor_ulps(floor_cs, ref_cs), name=f"wgrad {tag} {fam.name} colsum")


ONE_BLOCK_CASES = fb.wgrad_cases()[:-len(fb.WGRAD_TWO_SHAPES)]      # (the two-block shapes have their own test below)


@pytest.mark.parametrize("cls,shape,names", ONE_BLOCK_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else None)
def test_every_shape_class_and_family_is_inside_the_budget(cls, shape, names):
    from safe_marl_amd.nets import _wgrad_class
    k, m, n = shape
    assert _wgrad_class(m, n)[:2] == cls
    slabs, rpb = _split(k, m, n, _ws().numel())
    print(f"wgrad class {cls} shape {shape}: {_wgrad_class(m, n)[2]} column chunks, {slabs} slabs of {rpb} rows, the last of {k - (slabs - 1) * rpb}")
    if shape == fb.WGRAD_CAP_SHAPE:
        assert (k + 63) // 64 > 512 and slabs < 512 and 0 < k - (slabs - 1) * rpb < rpb and (k - (slabs - 1) * rpb) % 8 != 0
    fams = fb.wgrad_case(k, m, n)
    for nm in names:
        fam = _cuda(fams[nm])
        c, cs = _call(*fam.inputs)
        _held(c, cs, fam, f"{cls} {k}x{m}x{n}")


@pytest.mark.parametrize("k,m,n", [(2049, 64, 160), (515, 7, 161), (2053, 100, 64), (65, 32, 33)])
def test_two_runs_and_the_run_without_a_column_sum_give_the_same_bits(k, m, n):
    fam = _cuda(fb.wgrad_case(k, m, n)["offset"])
    c0, cs0 = _call(*fam.inputs)
    c1, cs1 = _call(*fam.inputs)
    assert torch.equal(c0, c1) and torch.equal(cs0, cs1)
    c2, _ = _call(*fam.inputs, colsum=False)
    assert torch.equal(c0, c2)


@pytest.mark.parametrize("k,m,n,family", [(2049, 64, 160, "plain"), (300, 65, 129, "offset"), (130, 4, 64, "halves"), (63, 33, 32, "mixed")])
def test_accumulate_adds_to_the_product_and_to_the_column_sum(k, m, n, family):
    """accumulate = 1 on a prefill of 1.0 (dW) and -2.0 (column sum): the result minus the prefill is inside the budget (the
    one rounding of the addition is half an ulp of the result's scale: inside FLOOR_ULPS)."""
    fam = _cuda(fb.wgrad_case(k, m, n)[family])
    c, cs = _call(*fam.inputs, accumulate=True, prefill=(1.0, -2.0))
    fresh_c, fresh_cs = _call(*fam.inputs)
    assert torch.equal(c, fresh_c + 1.0) and torch.equal(cs, fresh_cs - 2.0)
    _held(c - 1.0, cs + 2.0, fam, f"accumulate {k}x{m}x{n}")


@pytest.mark.parametrize("k,m,n", [(515, 7, 161), (513, 40, 149), (2053, 100, 64)])
@pytest.mark.parametrize("family", ["plain", "halves"])
def test_row_strided_operands_below_the_tile_width(k, m, n, family):
    """dy = rec[:, 5:5 + m] with m below the tile width 32 MT (7 < 32, 40 < 64, 100 < 192) and x a column slice alike, NaN in
    every other column of both records: the lanes past m load their neighbours' NaN into result rows that are never stored.
    Finite, inside the budget, and the bits of the call on contiguous copies — both calls split the rows alike (``_split``
    takes no pitch; the one place a pitch enters wgrad_prepare is the 2^31-byte limit of a block's view, far away here)."""
    fam = _cuda(fb.wgrad_case(k, m, n)[family])
    rec_a = torch.full((k, m + 11), float("nan"), device="cuda")
    rec_b = torch.full((k, n + 9), float("nan"), device="cuda")
    dy, x = rec_a[:, 5:5 + m], rec_b[:, 3:3 + n]
    dy.copy_(fam.inputs[0])
    x.copy_(fam.inputs[1])
    assert dy.stride(0) > m and x.stride(0) > n and _split(k, m, n, _ws().numel())[1] * max(m + 11, n + 9) * 4 < 2 ** 31
    c, cs = _call(dy, x)
    assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(cs).all())
    _held(c, cs, fam, f"strided {k}x{m}x{n}")
    dense_c, dense_cs = _call(*fam.inputs)
    assert torch.equal(c, dense_c) and torch.equal(cs, dense_cs)


@pytest.mark.parametrize("k,m,n", [(2053, 100, 64), (515, 7, 161), (1003, 64, 321), (257, 64, 20)])
def test_a_nan_and_an_inf_stay_in_their_row_and_column(k, m, n):
    """dy[k0, m0] = NaN, k0 an odd row of the last, partial slab: row m0 of dW and colsum[m0] are NaN, everything else has the
    bits of the run with 0 there.  x[k0, n0] = +Inf: column n0 of dW is not finite, everything else — the whole column sum —
    has the bits of the run with 0 there."""
    slabs, rpb = _split(k, m, n, _ws().numel())
    first = (slabs - 1) * rpb
    assert 0 < k - first < rpb
    k0 = first + 1 if first % 2 == 0 else first
    assert k0 % 2 == 1 and first <= k0 < k
    m0, n0 = m - 2 if m > 2 else 0, n - 1
    dy, x = (t.clone() for t in _cuda(fb.wgrad_case(k, m, n)["plain"]).inputs)
    dy[k0, m0] = 0.0
    base_c, base_cs = _call(dy, x)
    dy[k0, m0] = float("nan")
    c, cs = _call(dy, x)
    assert bool(c[m0].isnan().all()) and bool(cs[m0].isnan())
    others = torch.arange(m, device="cuda") != m0
    assert torch.equal(c[others], base_c[others]) and torch.equal(cs[others], base_cs[others])
    dy, x = (t.clone() for t in _cuda(fb.wgrad_case(k, m, n)["plain"]).inputs)
    x[k0, n0] = 0.0
    base_c, base_cs = _call(dy, x)
    x[k0, n0] = float("inf")
    c, cs = _call(dy, x)
    assert not bool(torch.isfinite(c[:, n0]).any())
    others = torch.arange(n, device="cuda") != n0
    assert torch.equal(c[:, others], base_c[:, others]) and torch.equal(cs, base_cs)


@pytest.mark.parametrize("k,m,n", [(513, 40, 149), (130, 4, 64), (2049, 64, 160)])
def test_b_row_cell_reads_the_window_of_a_larger_row_store(k, m, n):
    """x as rows cell .. cell + k - 1 of a store of R = k + 11 rows (row pitch n + 3), NaN outside the window, for cells 0, 3 and
    R - k written to the device cell between launches: the bits of the call on the window's own pointer without a cell."""
    fam = _cuda(fb.wgrad_case(k, m, n)["plain"])
    dy, x = fam.inputs
    R = k + 11
    cell = torch.zeros(1, dtype=torch.int64, device="cuda")
    for at in (0, 3, R - k):
        store = torch.full((R, n + 3), float("nan"), device="cuda")
        window = store[at:at + k, :n]
        window.copy_(x)
        cell.fill_(at)
        c, cs = _call(dy, window, cell=cell, b_base=store)
        want_c, want_cs = _call(dy, window)
        assert bool(torch.isfinite(c).all()) and torch.equal(c, want_c) and torch.equal(cs, want_cs)
        if at == 3:
            _held(c, cs, fam, f"b_row_cell {k}x{m}x{n}")


def _table():
    """Two problems per shape class (the first two shapes of fb.WGRAD_SHAPES: unequal k), the families spread over them, column
    sums for every other one, one accumulating."""
    problems = []
    shapes = [s for v in fb.WGRAD_SHAPES.values() for s in v[:2]]
    for i, (k, m, n) in enumerate(shapes):
        name = fb.WGRAD_FAMILIES[i % len(fb.WGRAD_FAMILIES)]
        fam = _cuda(fb.wgrad_case(k, m, n)[name])
        acc = i == 9
        out, cs = _guarded(m, n, 1.0 if acc else SENTINEL), _guarded(1, m, -2.0 if acc else SENTINEL)
        problems.append(dict(fam=fam, out=out, cs=cs, colsum=i % 2 == 1, accumulate=acc, shape=(k, m, n)))
    return problems


def _run_table(problems):
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import _wgrad_class
    need = []
    for p in problems:
        k, m, n = p["shape"]
        _, _, chunks, img = _wgrad_class(m, n)
        need.append(_lib.FLEXNET_WGRAD_CS_FLOATS + (k + 63) // 64 * chunks * img)
    ws = torch.empty(sum(need), device="cuda")
    table = (_lib.FlexWgradArgs * len(problems))()
    at = 0
    for a, p, floats in zip(table, problems, need):
        dy, x = p["fam"].inputs
        _problem(a, dy, x, p["out"][1], ws[at:at + floats], p["cs"][1] if p["colsum"] else None, p["accumulate"])
        at += floats
    _lib.launch("flexnet_wgrad_batched", table, len(problems))
    torch.cuda.synchronize()


def test_a_table_of_two_problems_per_class():
    from safe_marl_amd.nets import _wgrad_class
    runs = []
    for rep in range(2):
        problems = _table()
        assert len(problems) == 16 and sum(p["accumulate"] for p in problems) == 1
        assert sorted(_wgrad_class(p["shape"][1], p["shape"][2])[:2] for p in problems) == sorted(2 * list(fb.WGRAD_SHAPES))
        _run_table(problems)
        runs.append(problems)
    for p, q in zip(*runs):
        assert _guards_untouched(p["out"][0]) and _guards_untouched(p["cs"][0]), p["shape"]
        assert torch.equal(p["out"][0], q["out"][0]) and torch.equal(p["cs"][0], q["cs"][0])        # the same bits twice
        c, cs = p["out"][1], p["cs"][1][0]
        if not p["colsum"]:
            assert not p["accumulate"] and bool((p["cs"][0] == SENTINEL).all())
        if p["accumulate"]:
            c, cs = c - 1.0, cs + 2.0
        _held(c, cs if p["colsum"] else None, p["fam"], "batched %dx%dx%d" % p["shape"])


@pytest.mark.parametrize("k,m,n,n2", fb.WGRAD_TWO_SHAPES)
@pytest.mark.parametrize("family", fb.WGRAD_TWO_FAMILIES)
def test_the_second_input_block_is_inside_the_budget(k, m, n, n2, family):
    """[x | x2] from their two homes as one operand (nets.tall_wgrad's x2 / out2, class [2, 5]): both output blocks — column
    blocks of one guarded gradient, five untouched columns between them — and the column sum."""
    from safe_marl_amd.nets import tall_wgrad
    fam = _cuda(fb.wgrad_case(k, m, n + n2)[family])
    dy, both = fam.inputs
    x, x2 = both[:, :n].contiguous(), both[:, n:].contiguous()
    buf, dW = _guarded(m, n + 5 + n2)
    cbuf, cs = _guarded(1, m)
    tall_wgrad(dy, x, out=dW[:, :n], colsum=cs[0], x2=x2, out2=dW[:, n + 5:])
    torch.cuda.synchronize()
    assert _guards_untouched(buf) and _guards_untouched(cbuf) and bool((dW[:, n:n + 5] == SENTINEL).all())
    _held(torch.cat((dW[:, :n], dW[:, n + 5:]), 1), cs[0], fam, f"two blocks {k}x{m}x({n}|{n2})")
