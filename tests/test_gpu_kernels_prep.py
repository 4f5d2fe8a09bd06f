"""Kernel-level checks of the load-time and per-batch preparation (csrc/k_prep.hip):
k_rows_to_i8, k_rows_to_i8_sample and k_query_prep against the float64 models of tests/kcheck.py,
called through the test-only shim within the contract index.cpp establishes.

What a wrong kernel here would do silently: certification assumes that ea_max
bounds EVERY row's quantisation error and that ebound[q] is built from it; an ea_max that missed a
block, a wave's quarter of a block or the appended rows would still give exact results on almost
all data.  So the worst row is planted at each position a reduction could miss.
"""
import numpy as np
import pytest

import kcheck as kc

pytestmark = pytest.mark.gpu

MAX_EXCUSED = 4  # per case (a condition of the issue, not a measurement); the seeds give 0


def _check_rows_case(a, plant):
    """One k_rows_to_i8 launch against the model; returns (ea_max, E, excused)."""
    n, dim = a.shape
    op, sc, ea = kc.rows_to_i8(a)
    n_pad, ld = op.shape
    assert not op[:, dim:].any(), "pad columns (dim <= c < ld) must be zero"
    assert not op[n:].any(), "pad rows (n <= r < n_pad) must be zero"
    nb = (n + 31) // 32
    assert np.all(sc[nb:] == 1.0), "blocks of pad rows take scale 1.0"
    excused = kc.compare_quant(a, 32, op[:n, :dim], sc[:nb])
    assert excused <= MAX_EXCUSED
    # E = max e_row in float64 from the GPU's own operand and scales
    e = kc.quant_err(kc.unit_rows(a), np.repeat(sc[:nb], 32)[:n], op[:n, :dim])
    E = float(e.max())
    if plant is not None:
        assert int(np.argmax(e)) == plant, "test data: the planted row must be the worst row"
    assert np.isfinite(ea) and float(ea) >= E, f"ea_max {ea!r} below the worst row's error {E!r} (row {int(np.argmax(e))})"
    assert float(ea) <= E * (1 + 1e-6) + 1e-9, f"ea_max {ea!r} is not tight: E = {E!r}"
    return ea, E, excused


@pytest.mark.parametrize("dim", kc.PREP_DIMS)
def test_rows_to_i8_operand_scales_and_ea_max(gpu, dim):
    """Every n of PREP_NS with the worst row planted at row 0, row n - 1 and (n >= 96) local rows
    0 / 8 / 16 / 24 / 31 of a middle block; each corpus holds a zero row and rows whose sums of
    squares are 1e-36 and 1e36 (from 13 rows)."""
    total = 0
    for n in kc.PREP_NS:
        for plant in kc.plant_positions(n):
            a = kc.prep_rows(n, dim, plant)
            if n > 12 and plant not in (1, 5, 9):
                ss = np.sum(a[[1, 5, 9]].astype(np.float64) ** 2, axis=1)
                assert ss[0] == 0 and abs(ss[1] / 1e-36 - 1) < 1e-5 and abs(ss[2] / 1e36 - 1) < 1e-5
            _, _, ex = _check_rows_case(a, plant)
            total += ex
    print(f"rows_to_i8 dim {dim}: {total} excused elements")


@pytest.mark.parametrize("kind", ("b", "c"))
def test_rows_to_i8_outlier_and_positive_data(gpu, kind):
    for dim, n in kc.PREP_KIND_CASES:
        _, _, ex = _check_rows_case(kc.prep_rows(n, dim, None, kind), None)
        print(f"rows_to_i8 data ({kind}) dim {dim}: {ex} excused elements")


@pytest.mark.parametrize("dim", kc.PREP_DIMS)
def test_rows_to_i8_sample_operand(gpu, dim):
    """The sample operand: corpus rows 0, 32, 64, ... contiguous, one scale per 128 of them, zero
    rows up to n_s_pad."""
    total = 0
    for n in kc.PREP_SAMPLE_NS:
        a = kc.prep_rows(n, dim, kc.plant_positions(n)[-1])
        op, sc = kc.rows_to_i8_sample(a)
        smp = a[::32]
        n_s = smp.shape[0]
        assert n_s == (n + 31) // 32 and op.shape[0] == kc.round_up(n_s, 128)
        assert not op[:, dim:].any() and not op[n_s:].any()
        ex = kc.compare_quant(smp, 128, op[:n_s, :dim], sc)
        assert ex <= MAX_EXCUSED
        total += ex
    print(f"rows_to_i8_sample dim {dim}: {total} excused elements")


# ---- the same bound through the ABI ------------------------------------------------------------
def _row_ebound(bsr_mod, parts, dim, dtype=None):
    ix = bsr_mod.Index(dim, max_k=8, device=0, **({} if dtype is None else {"dtype": dtype}))
    try:
        ix.load(parts[0])
        for p in parts[1:]:
            ix.append_many(p)
        q = np.ones((1, dim), np.float32)
        ix.local_top_k(q, 1)
        return np.float32(ix.last_stats().row_ebound)
    finally:
        ix.close()


@pytest.mark.parametrize("where,n_a", (("a", 300), ("b", 300), ("b", 256), ("a", 77)))
def test_row_ebound_after_append_equals_whole_load(gpu, bsr_mod, where, n_a):
    """last_stats().row_ebound after load(a) + append_many(b) has the bits it has after load(a || b)
    -- and those are the model's: the worst row in a, in b, and with len(a) % 32 != 0."""
    dim, n_b = 130, 200
    n = n_a + n_b
    plant = 40 if where == "a" else n_a + 150
    rows = kc.prep_rows(n, dim, plant)
    whole = _row_ebound(bsr_mod, [rows], dim)
    split = _row_ebound(bsr_mod, [rows[:n_a], rows[n_a:]], dim)
    assert whole.view(np.uint32) == split.view(np.uint32), (whole, split)
    _, _, e = kc.quantize(rows, 32)
    assert int(np.argmax(e)) == plant
    E = float(e.max())
    assert E <= float(whole) <= E * (1 + 1e-6) + 1e-9


def test_row_ebound_bf16_corpus(gpu, bsr_mod):
    """A BSR_BF16 corpus: the bound is the model's on the widened rows."""
    dim, n = 130, 333
    rows = kc.prep_rows(n, dim, 170)
    bits = (rows.view(np.uint32) >> np.uint32(16)).astype(np.uint16)  # truncation: any bf16 values do
    widened = (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    got = _row_ebound(bsr_mod, [bits], dim, dtype=bsr_mod.BSR_BF16)
    split = _row_ebound(bsr_mod, [bits[:100], bits[100:]], dim, dtype=bsr_mod.BSR_BF16)
    assert got.view(np.uint32) == split.view(np.uint32)
    E = float(kc.quantize(widened, 32)[2].max())
    assert E <= float(got) <= E * (1 + 1e-6) + 1e-9


# ---- query preparation --------------------------------------------------------------------------
def _check_query_prep(q, ea, with_op):
    nq, dim = q.shape
    o = kc.query_prep(q, ea, with_op=with_op, status_in=0x10)
    qpad, ld = o["qpad"], o["ld"]
    c = kc.consts()
    # the padded f32 copy, bit for bit (a NaN keeps its payload), zeros past dim and past nq
    want = np.zeros((qpad, ld), np.float32)
    want[:nq, :dim] = q
    assert np.array_equal(o["qf32"].view(np.uint32), want.view(np.uint32))
    # |b|: sequential f32 sum of squares from -0.0, correctly rounded sqrt
    nb = kc.seq_norm_f32(q)
    fin = ~np.isnan(nb)
    assert np.array_equal(o["nb"][:nq][fin].view(np.uint32), nb[fin].view(np.uint32))
    assert np.isnan(o["nb"][:nq][~fin]).all() and not o["nb"][nq:].any()
    flags = kc.query_flags(q, nb)
    assert np.array_equal(o["qflags"][:nq], flags) and np.all(o["qflags"][nq:] == kc.Q_NOAPPROX)
    assert np.array_equal(o["qids"], np.minimum(np.arange(qpad), nq - 1))
    # the status word: only the kQueryNonFinite bit is checked, the one the host acts on.  (kernels.hpp
    # says the word receives the OR of the flags; k_query_prep ORs only that bit -- DESIGN.md §2.)
    # The other status words are not touched.
    want_bit = np.bitwise_or.reduce(flags) & kc.Q_NONFINITE
    word = int(o["status"][c.st_query_flags])
    assert (word & kc.Q_NONFINITE) == int(want_bit)
    assert (word & ~(kc.Q_NONFINITE | kc.Q_NOAPPROX)) == 0x10
    others = np.delete(o["status"], c.st_query_flags)
    assert np.all(others == 0x10)
    if not with_op:
        # exact scan only: no operand, scale or bound is written
        assert np.all(o["qop"] == 0x5A) and np.isnan(o["qscale"]).all() and np.isnan(o["ebound"]).all()
        return 0
    ok = np.zeros(qpad, bool)
    ok[:nq] = flags == 0
    assert not o["qop"][~ok].any(), "a padding / no-approx query gets a zero operand (every column)"
    assert not o["qscale"][~ok].any() and np.all(np.isposinf(o["ebound"][~ok]))
    assert not o["qop"][:, dim:].any()
    rows = np.flatnonzero(ok)
    excused = kc.compare_quant(q[rows], 1, o["qop"][rows, :dim], o["qscale"][rows])
    assert excused <= MAX_EXCUSED
    eb = kc.quant_err(kc.unit_rows(q[rows]), o["qscale"][rows], o["qop"][rows, :dim])
    lo = kc.ebound_model(ea, eb)
    # the kernel: f32_round_up(E(eb')) with eb' = eb (1 + 1e-9) + 1e-12; twice that slack covers its
    # different summation order, and no further ulp is allowed
    hi = kc.ebound_model(ea, eb * (1 + 2e-9) + 2e-12)
    got = o["ebound"][rows]
    assert np.all(got.astype(np.float64) >= lo), "ebound below ea + eb + ea eb + 1.5e-4"
    assert np.all(got <= kc.f32_round_up(hi)), "ebound above the rounded-up bound with the kernel's slack"
    return excused


@pytest.mark.parametrize("dim", kc.QUERY_DIMS)
@pytest.mark.parametrize("with_op", (True, False))
def test_query_prep(gpu, dim, with_op):
    """nq = 3 (qpad 16; two variants, see kcheck.special_queries) and nq = 300 (qpad 512), each with
    zero, 1e-25, 1e19 and NaN queries.  dim 8256: the row is not staged in LDS and the operand's
    second char4 pass is live."""
    ea = np.float32(0.004321)
    total = 0
    for nq, variant in kc.QUERY_BATCHES:
        q = kc.prep_queries(nq, dim, variant=variant)
        sp = kc.special_queries(nq, variant)
        flags = kc.query_flags(q, kc.seq_norm_f32(q))
        for name, want in (("zero", 2), ("tiny", 2), ("huge", 2), ("nan", 3)):
            if name in sp:
                assert flags[sp[name]] == want, name
        assert (flags == 0).any()
        total += _check_query_prep(q, ea, with_op)
    print(f"query_prep dim {dim} with_op {with_op}: {total} excused elements")


@pytest.mark.parametrize("kind", ("b", "c"))
def test_query_prep_outlier_and_negative_queries(gpu, kind):
    for dim in kc.QUERY_KIND_DIMS:
        ex = _check_query_prep(kc.prep_queries(40, dim, kind), np.float32(0.0123), True)
        print(f"query_prep data ({kind}) dim {dim}: {ex} excused elements")
