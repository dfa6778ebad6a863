"""csrc/linear.hip (flexnet_linear2, the centralised critic's first layer) under the fp64 error budget of tests/fp64_budget.py
(DESIGN.md §5), called directly — nets.critic_first_layer launches it only from 8 192 rows: out = bias + x1 W1^T + x2 W2^T against
the same formula in fp64, the yardstick the fp32 composition on the GPU (two library GEMMs), the floor ``fb.linear2_sum_rounding``.
Rows from one to 2 049 (below, at and past one 32-row tile), widths on both sides of every step of the kernel's ``SS``
instantiations, k2 = 0 and k2 = 4 mod 8, NaN in the id columns of W the kernel must skip, six input families from a CPU
generator (tests/test_fp64_budget_cpu.py holds their conditions), the output between sentinel guard rows."""
import ctypes as C

import pytest
import torch

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
GUARD = 3


def _guarded(rows):
    buf = torch.full((rows + 2 * GUARD, 64), SENTINEL, device="cuda")
    return buf, buf[GUARD:GUARD + rows]


def _args(bias, x1, x2, W, out, k1, k2, cell=None, x1_base=None):
    from safe_marl_amd import _lib
    a = _lib.FlexLinear2Args()
    a.rows, a.k1, a.k2 = x1.shape[0], k1, k2
    a.ld1 = x1.stride(0) if x1.shape[0] > 1 else max(x1.stride(0), k1)
    a.ld2 = 0 if k2 == 0 else (x2.stride(0) if x2.shape[0] > 1 else max(x2.stride(0), k2))
    a.ldw, a.c1, a.c2 = W.stride(0), 0, k1 + fb.LINEAR2_ID_COLUMNS
    a.x1, a.x2 = x1.data_ptr(), None if k2 == 0 else x2.data_ptr()
    a.w, a.bias, a.out = W.data_ptr(), bias.data_ptr(), out.data_ptr()
    if cell is not None:
        a.x1, a.x1_row_cell = x1_base.data_ptr(), cell.data_ptr()
    return a


def _call(bias, x1, x2, W, k1, k2, **kw):
    """One flexnet_linear2 launch into a guarded output: out [rows, 64], a copy."""
    from safe_marl_amd import _lib
    buf, out = _guarded(x1.shape[0])
    _lib.launch("flexnet_linear2", _args(bias, x1, x2, W, out, k1, k2, **kw))
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all()), (x1.shape, k1, k2)
    return out.clone()


def _held(got, fam, k1, k2, tag):
    bias, x1, x2, W = fam.inputs
    c2 = k1 + fb.LINEAR2_ID_COLUMNS
    ref = fb.linear2_plain(bias.double(), x1.double(), x2.double(), W.double(), 0, c2)
    yard = fb.linear2_plain(bias, x1, x2, W, 0, c2)
    floor = fb.linear2_sum_rounding(x1, x2, W, 0, c2, fam.params.get("split"))
    fb.within_budget(got, yard, ref, floor_ulps=fb.floor_ulps(floor, ref), name=f"linear2 {tag} {fam.name}")


def _cuda(fam):
    return fb.Family(fam.name, tuple(t.cuda() for t in fam.inputs), fam.params, fam.groups)


@pytest.mark.parametrize("k1,k2", fb.LINEAR2_WIDTHS)
def test_every_width_row_count_and_family_is_inside_the_budget(k1, k2):
    ss = fb.linear2_ss(k1, k2)
    assert ss == {8: 1, 12: 1, 148: 1, 256: 1, 264: 2, 444: 2, 512: 2, 520: 3, 740: 3, 768: 3}[k1 + k2]
    print(f"linear2 widths ({k1}, {k2}): SS = {ss}")
    for rows in fb.LINEAR2_ROWS:
        for fam in fb.linear2_case(rows, k1, k2).values():
            fam = _cuda(fam)
            out = _call(*fam.inputs, k1, k2)
            _held(out, fam, k1, k2, f"SS{ss} {rows}x({k1}+{k2})")
            assert torch.equal(out, _call(*fam.inputs, k1, k2))                     # fixed summation order: the same bits
            if fam.name == "zero_x":
                assert torch.equal(out, fam.inputs[0].expand(rows, 64))


@pytest.mark.parametrize("family", ["plain", "halves"])
def test_row_strided_inputs(family):
    """x1 and x2 as column slices of wider records (pitches multiples of 4, bases 16-byte aligned), NaN in the padding columns:
    the bits of the call on contiguous copies."""
    rows, k1, k2 = 97, 432, 12
    fam = _cuda(fb.linear2_case(rows, k1, k2)[family])
    bias, x1, x2, W = fam.inputs
    rec1 = torch.full((rows, k1 + 8), float("nan"), device="cuda")
    rec2 = torch.full((rows, k2 + 8), float("nan"), device="cuda")
    s1, s2 = rec1[:, 4:4 + k1], rec2[:, 4:4 + k2]
    s1.copy_(x1)
    s2.copy_(x2)
    out = _call(bias, s1, s2, W, k1, k2)
    assert bool(torch.isfinite(out).all())
    _held(out, fam, k1, k2, f"strided {rows}x({k1}+{k2})")
    assert torch.equal(out, _call(bias, x1, x2, W, k1, k2))


@pytest.mark.parametrize("k1,k2", [(8, 4), (144, 4), (432, 12), (720, 20), (736, 32), (256, 8)])
@pytest.mark.parametrize("rows", [33, 97])
def test_a_nan_row_and_an_inf_row_stay_in_their_rows(rows, k1, k2):
    """Row r0 has a NaN in one observation column: output row r0 is NaN in all 64 units.  Row r1 has +Inf in the last four
    action columns — with k2 = 4 mod 8 the piece the kernel reads a second time, clamped, against zero weights (0 * Inf): output
    row r1 is not finite.  Every other row, the tile neighbours of both included, has the bits of the run with zeros there.

    The fp64 reference has +-Inf in row r1 (or NaN where +Inf and -Inf meet); the kernel has NaN in ALL 64 units of row r1
    where k2 = 4 mod 8, from the 0 * Inf of the second read — recorded, not a failure: the row is not finite either way."""
    fam = _cuda(fb.linear2_case(rows, k1, k2)["plain"])
    bias, x1, x2, W = (t.clone() for t in fam.inputs)
    r0, r1 = rows - 2, 1 if rows < 64 else 32
    x1[r0, k1 // 2] = 0.0
    x2[r1, k2 - 4:] = 0.0
    base = _call(bias, x1, x2, W, k1, k2)
    assert bool(torch.isfinite(base).all())
    x1[r0, k1 // 2] = float("nan")
    x2[r1, k2 - 4:] = float("inf")
    out = _call(bias, x1, x2, W, k1, k2)
    assert bool(out[r0].isnan().all())
    assert not bool(torch.isfinite(out[r1]).any())
    ref = fb.linear2_plain(bias.double(), x1.double(), x2.double(), W.double(), 0, k1 + fb.LINEAR2_ID_COLUMNS)
    assert not bool(torch.isfinite(ref[r1]).any())
    print(f"linear2 {rows}x({k1}+{k2}) Inf row: kernel NaN in {int(out[r1].isnan().sum())} units, fp64 reference in {int(ref[r1].isnan().sum())}")
    others = torch.ones(rows, dtype=torch.bool, device="cuda")
    others[r0] = others[r1] = False
    assert torch.equal(out[others], base[others])


@pytest.mark.parametrize("rows,k1,k2", [(33, 144, 4), (97, 512, 8), (2049, 720, 20)])
def test_x1_row_cell_reads_the_window_of_a_larger_row_store(rows, k1, k2):
    """x1 as rows cell .. cell + rows - 1 of a store of R = rows + 11 rows (pitch k1 + 4), NaN outside the window, for cells 0, 3
    and R - rows written to the device cell between launches: the bits of the call on the window's own pointer."""
    fam = _cuda(fb.linear2_case(rows, k1, k2)["plain"])
    bias, x1, x2, W = fam.inputs
    R = rows + 11
    cell = torch.zeros(1, dtype=torch.int64, device="cuda")
    for at in (0, 3, R - rows):
        store = torch.full((R, k1 + 4), float("nan"), device="cuda")
        window = store[at:at + rows, :k1]
        window.copy_(x1)
        cell.fill_(at)
        out = _call(bias, window, x2, W, k1, k2, cell=cell, x1_base=store)
        assert bool(torch.isfinite(out).all()) and torch.equal(out, _call(bias, window, x2, W, k1, k2))
        if at == 3:
            _held(out, fam, k1, k2, f"x1_row_cell {rows}x({k1}+{k2})")


def test_refusals_launch_nothing():
    """k1 not a multiple of 8, more than 768 input columns, a misaligned ``out``: FLEXNET_EUNSUPPORTED from the host checks, the
    output untouched."""
    from safe_marl_amd import _lib
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = 40
    x1 = torch.randn(rows, 776, device="cuda")
    x2 = torch.randn(rows, 8, device="cuda")
    W = torch.randn(64, 776 + fb.LINEAR2_ID_COLUMNS + 8, device="cuda")
    bias = torch.randn(64, device="cuda")
    buf = torch.full((rows + 2 * GUARD, 64), SENTINEL, device="cuda")
    out = buf[GUARD:GUARD + rows]
    assert fb.linear2_ss(768, 8) == 4
    for k1, k2, shift in ((12, 8, 0), (768, 8, 0), (16, 8, 1)):
        a = _args(bias, x1, x2, W, out.view(-1)[shift:], k1, k2)
        assert lib.flexnet_linear2(C.byref(a), stream) == _lib.FLEXNET_EUNSUPPORTED, (k1, k2, shift)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    a = _args(bias, x1, x2, W, out, 16, 8)                                           # ... and the aligned call of that width runs
    assert lib.flexnet_linear2(C.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())
