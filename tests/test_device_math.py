"""The device-side arithmetic primitives, called directly (rt_debug_device_math, include/rt_mi355.h) and compared BIT FOR BIT
with plain references: csrc/rt_fastmath.h (rtf::rcp, rcp3, sqrt, rcp_sqrt, div2, div3 and their *_fast paths and guards), the
device instantiation of csrc/rt_mesa_math.h (rtm::sin_, cos_, tan_, exp_) and the helpers of csrc/rt_kernels.hip (f2h_rtz,
half_bits_to_float, pow5, halton_eval).  The rendered pixels only ever show these functions on the operands the test scenes
produce; here they see every exponent, the guard boundaries, denormals, infinities and NaN.

Every comparison is on uint32 bit patterns.  The one relaxation: any NaN equals any NaN.  +0 and -0 differ.  No tolerance
appears anywhere in this file.

The entry runs record i in lane i % 64 of wavefront i / 64, so the arrays below decide which operands share a wavefront.
That matters for the rtf:: functions: they take the IEEE sequence for a WHOLE wavefront as soon as one of its lanes needs it.
Each rtf test therefore holds a `pure` section (aligned groups of 64 interior operands: nobody votes, the value returned IS the
fast path's), `mixed` sections (the same operands with one fallback-needing lane, and 63 such lanes around one interior
operand: everybody takes the IEEE sequence) and is run again with the last wavefront cut short.  The division tests add
whole wavefronts with +-0 numerators, which the fast path answers itself without a vote.

This file is the regression gate; tools/fastmath_exhaustive.hip is the full 2^32 sweep, run by hand."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0xDEADBEEF)
MANTS = np.array([0, 1, 2, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF], dtype=np.uint32)
SIGN = np.uint32(0x80000000)
PURE_WAVES = 1024       # wavefronts of the pure section
MIXED_WAVES = 256       # wavefronts of each mixed group (the first MIXED_WAVES pure wavefronts, one or 63 lanes replaced)


# ---- bit helpers -------------------------------------------------------------------------------
def f32(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def u32(f):
    f = np.ascontiguousarray(f)
    assert f.dtype == np.float32, f.dtype        # a float64 that slipped in would compare rounded twice
    return f.view(np.uint32)


def same(got, want):
    """Equal bit patterns, or both NaN."""
    return (got == want) | (np.isnan(f32(got)) & np.isnan(f32(want)))


def check(got, want, what, inputs=None):
    got = np.ascontiguousarray(got, dtype=np.uint32)
    want = u32(want) if np.asarray(want).dtype == np.float32 else np.ascontiguousarray(want, dtype=np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = same(got, want)
    if ok.all():
        return
    bad = np.flatnonzero(~ok)
    lines = []
    for i in bad[:8]:
        src = "" if inputs is None else " in " + " ".join(f"{int(v):08x}" for v in np.atleast_1d(inputs[i]))
        lines.append(f"  record {int(i)} (lane {int(i) % 64}){src}: got {int(got[i]):08x} want {int(want[i]):08x}")
    pytest.fail(f"{what}: {len(bad)} of {len(ok)} differ\n" + "\n".join(lines))


def rand_bits(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def with_exp(u, lo, span):
    """u's sign and mantissa under an exponent field in [lo, lo + span)."""
    return (u & np.uint32(0x807FFFFF)) | ((np.uint32(lo) + ((u >> np.uint32(23)) & np.uint32(0xFF)) % np.uint32(span)) << np.uint32(23))


def near(x, k=4):
    """The bit patterns within k ulps of float32 x, both signs."""
    b = int(u32(np.array([x], dtype=np.float32))[0] & 0x7FFFFFFF)
    p = np.arange(max(b - k, 0), b + k + 1, dtype=np.uint32)
    return np.concatenate([p, p | SIGN])


@functools.lru_cache(None)
def structured_core():
    """Every exponent field x the eight boundary mantissas, both signs."""
    e = np.arange(256, dtype=np.uint32)
    pos = ((e[:, None] << np.uint32(23)) | MANTS[None, :]).ravel()
    out = np.concatenate([pos, pos | SIGN])
    out.setflags(write=False)
    return out


@functools.lru_cache(None)
def structured_bits():
    """The structured set: structured_core() and 2^20 random bit patterns."""
    out = np.concatenate([structured_core(), rand_bits(np.random.default_rng(0x5EED), 1 << 20)])
    out.setflags(write=False)
    return out


def records(*cols):
    n = len(cols[0])
    r = np.zeros((n, 4), dtype=np.uint32)
    for k, c in enumerate(cols):
        r[:, k] = c
    return r


# ---- the host's arithmetic is the reference: check it before trusting it ---------------------------
def assert_host_keeps_denormals():
    tiny = np.array([1e-40], dtype=np.float32)
    prod = tiny * np.float32(1)
    assert u32(prod)[0] == u32(tiny)[0] == 0x000116C2, \
        "this HOST flushes float32 denormals: numpy is no IEEE reference here (a property of the host, not of the kernels)"


def ref_div(num, den):
    """Correctly rounded float32 num / den, cross-checked against the float64 quotient rounded once more (innocuous double
    rounding: 53 >= 2 * 24 + 2)."""
    assert_host_keeps_denormals()
    with np.errstate(all="ignore"):
        q = num / den
        q64 = (num.astype(np.float64) / den.astype(np.float64)).astype(np.float32)
    assert q.dtype == np.float32
    assert same(u32(q), u32(q64)).all(), "this HOST's float32 division is not correctly rounded: no reference (host problem)"
    return q


def ref_sqrt(x):
    assert_host_keeps_denormals()
    with np.errstate(all="ignore"):
        s = np.sqrt(x)
        s64 = np.sqrt(x.astype(np.float64)).astype(np.float32)
    assert s.dtype == np.float32
    assert same(u32(s), u32(s64)).all(), "this HOST's float32 sqrt is not correctly rounded: no reference (host problem)"
    return s


def ref_rcp(x):
    return ref_div(np.ones_like(x), x)


def ref_rcp_sqrt(x):
    return ref_rcp(ref_sqrt(x))         # the two-step form: RN(1 / RN(sqrt x))


# ---- wavefront composition -----------------------------------------------------------------------
class Layout:
    """records [n, 4] and the named, 64-aligned sections they consist of; `interior` marks the records built from interior
    operands only, `fallback` those holding an operand that needs the IEEE sequence."""

    def __init__(self, general, interior, fallback, seed, quiet=None):
        """quiet: records that are not interior yet must not vote either (whole wavefronts of them form a section)."""
        rng = np.random.default_rng(seed)
        assert len(interior) >= 64 * PURE_WAVES and len(fallback) >= 64
        pad = (-len(general)) % 64
        general = np.concatenate([general, interior[:pad]])
        pure = interior[: 64 * PURE_WAVES]
        base = pure[: 64 * MIXED_WAVES].reshape(MIXED_WAVES, 64, 4)
        pick = lambda n: fallback[rng.integers(0, len(fallback), n)]
        waves = np.arange(MIXED_WAVES)
        parts = [("general", general, None), ("pure", pure, None)]
        if quiet is not None:
            assert len(quiet) % 64 == 0
            parts.append(("pure, zero numerators", quiet, np.zeros(len(quiet), bool)))
        for name, lanes in (("mixed lane 0", np.zeros(MIXED_WAVES, int)), ("mixed random lane", rng.integers(0, 64, MIXED_WAVES)),
                            ("mixed 63 fallback lanes", None), ("mixed lane 63", np.full(MIXED_WAVES, 63))):
            w = base.copy()
            fb = np.zeros((MIXED_WAVES, 64), bool)
            if lanes is None:                       # 63 fallback operands around one interior operand
                keep = rng.integers(0, 64, MIXED_WAVES)
                fb[:] = True
                fb[waves, keep] = False
                w[fb] = pick(int(fb.sum()))
            else:
                fb[waves, lanes] = True
                w[waves, lanes] = pick(MIXED_WAVES)
            parts.append((name, w.reshape(-1, 4), fb.ravel()))
        self.records = np.ascontiguousarray(np.concatenate([p[1] for p in parts]))
        self.sections, self.interior, self.fallback = {}, np.zeros(len(self.records), bool), np.zeros(len(self.records), bool)
        at = 0
        for name, recs, fb in parts:
            assert at % 64 == 0
            self.sections[name] = slice(at, at + len(recs))
            if name == "pure, zero numerators":
                self.quiet = slice(at, at + len(recs))
            elif name != "general":
                self.fallback[at:at + len(recs)] = fb if fb is not None else False
                self.interior[at:at + len(recs)] = ~fb if fb is not None else True
            at += len(recs)
        assert len(self.records) % 64 == 0 and len(self.records) <= 1 << 22     # the last wavefront is the one that gets cut
        # the last wavefront holds its fallback operand in lane 63: n - 1 turns it into a pure wavefront
        assert self.fallback[-1] and not self.fallback[-64:-1].any()
        self.records.setflags(write=False)


def run_ragged(tracer, op, recs):
    """The whole array, then cut to n - 1 and n - 63 records: [(m, out[:m])].  Nothing past record m - 1 may be written."""
    n = len(recs)
    runs = []
    for m in (n, n - 1, n - 63):
        out = np.full((n + 64, 4), SENTINEL, dtype=np.uint32)
        got = tracer.device_math(op, recs, n=m, out=out)
        assert got.shape == (n + 64, 4)
        assert (got[m:] == SENTINEL).all(), f"{op}: n = {m} wrote past its last record"
        runs.append((m, got[:m]))
    return runs


def check_sections(tracer, op, lay, wants):
    """wants: {output word: float32 reference}.  Every section, whole and ragged, bit for bit."""
    for m, got in run_ragged(tracer, op, lay.records):
        for name, sl in lay.sections.items():
            sl = slice(sl.start, min(sl.stop, m))
            for col, want in wants.items():
                check(got[sl, col], want[sl], f"{op} word {col}, section '{name}', n = {m}", lay.records[sl])
        used = set(wants)
        for col in set(range(4)) - used - set(FAST_WORDS.get(op, ())):
            assert (got[:, col] == 0).all(), f"{op}: unused output word {col} is not 0"


FAST_WORDS = {"rcp": (1, 2), "sqrt": (1, 2), "rcp_sqrt": (1, 2), "div2": (2, 3)}


# ---- operands ------------------------------------------------------------------------------------
def rcp_interior(rng, n):
    """2^-125 <= |x| <= 2^125, the two ends included."""
    u = with_exp(rand_bits(rng, n), 2, 250)          # fields 2 .. 251, any mantissa
    u[:4] = [0x01000000, 0x81000000, 0x7E000000, 0xFE000000]     # +-2^-125, +-2^125
    return u


def rcp_fallback(rng, n):
    """No normal reciprocal: +-0, +-inf, NaN, denormals below 2^-128 (1/x overflows), |x| >= 1.5 * 2^126 (1/x is denormal)."""
    r = rand_bits(rng, n)
    kinds = [np.uint32(0), SIGN, np.uint32(0x7F800000), np.uint32(0xFF800000), np.uint32(0x7FC00000),
             (r & np.uint32(0x801FFFFF)) | np.uint32(1), (r & np.uint32(0x807FFFFF)) | np.uint32(0x7F000000),
             (r & np.uint32(0x807FFFFF)) | np.uint32(0x7EC00000)]
    sel = rng.integers(0, len(kinds), n)
    return np.choose(sel, kinds).astype(np.uint32)


def sqrt_interior(rng, n):
    """2^-99 <= x <= 2^126."""
    u = with_exp(rand_bits(rng, n), 28, 225) & np.uint32(0x7FFFFFFF)      # fields 28 .. 252
    u[:2] = [0x0E000000, 0x7E800000]                                       # 2^-99, 2^126
    return u


def sqrt_fallback(rng, n):
    """Outside [2^-100, inf): +-0, denormals, tiny normals, negatives, +-inf, NaN."""
    r = rand_bits(rng, n)
    kinds = [np.uint32(0), SIGN, np.uint32(0x7F800000), np.uint32(0xFF800000), np.uint32(0x7FC00000),
             r & np.uint32(0x007FFFFF), with_exp(r, 1, 26) & np.uint32(0x7FFFFFFF), r | SIGN, np.uint32(0x0D7FFFFF)]
    sel = rng.integers(0, len(kinds), n)
    return np.choose(sel, kinds).astype(np.uint32)


def div_interior(rng, n):
    """Exponents within +-40 of 1.0 (fields 87 .. 167): never zero, every quotient normal."""
    return with_exp(rand_bits(rng, n), 87, 81)


def div_bad_den(rng, n):
    """Denominators whose reciprocal is no normal number: +-0, +-inf, NaN, denormals below 2^-128."""
    r = rand_bits(rng, n)
    kinds = [np.uint32(0), SIGN, np.uint32(0x7F800000), np.uint32(0xFF800000), np.uint32(0x7FC00000), np.uint32(0xFFC00001),
             (r & np.uint32(0x801FFFFF)) | np.uint32(1)]
    return np.choose(rng.integers(0, len(kinds), n), kinds).astype(np.uint32)


def tiny_num(rng, n):
    """Nonzero numerators below 2^-100: denormals and the smallest normals."""
    r = rand_bits(rng, n)
    return np.where(r & np.uint32(1 << 30), (r & np.uint32(0x807FFFFF)) | np.uint32(1), with_exp(r, 1, 26)).astype(np.uint32)


@functools.lru_cache(None)
def rcp_layout():
    rng = np.random.default_rng(101)
    extra = [near(np.float32(2.0 ** e)) for e in (126, -126, 127, -127, -128)]     # where 1/x turns denormal or overflows
    general = records(np.concatenate([structured_bits()] + extra))
    return Layout(general, records(rcp_interior(rng, 64 * PURE_WAVES)), records(rcp_fallback(rng, 4096)), 102)


@functools.lru_cache(None)
def rcp3_layout():
    rng = np.random.default_rng(111)
    a = np.concatenate([structured_bits()] + [near(np.float32(2.0 ** e)) for e in (126, -126, 127, -127, -128)])
    general = records(a, np.roll(a, 1), np.roll(a, 4099))
    n = 64 * PURE_WAVES
    interior = records(rcp_interior(rng, n), rcp_interior(rng, n)[::-1], np.roll(rcp_interior(rng, n), 7))
    fallback = interior[:4098].copy()
    fallback[np.arange(4098), np.arange(4098) % 3] = rcp_fallback(rng, 4098)       # one component of three
    return Layout(general, interior, fallback, 112)


@functools.lru_cache(None)
def sqrt_layout():
    rng = np.random.default_rng(121)
    extra = [near(np.float32(2.0 ** -100)), np.array([0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF], dtype=np.uint32)]
    general = records(np.concatenate([structured_bits()] + extra))
    return Layout(general, records(sqrt_interior(rng, 64 * PURE_WAVES)), records(sqrt_fallback(rng, 4096)), 122)


def structured_mants(rng, n):
    """tools/fastmath_exhaustive.hip's structured_mant: seven boundary mantissas and a random one."""
    table = np.array([0, 1, 0x7FFFFF, 0x7FFFFE, 0x400000, 0x3FFFFF, 0x400001], dtype=np.uint32)
    sel = rng.integers(0, 8, n)
    return np.where(sel < 7, table[np.minimum(sel, 6)], rand_bits(rng, n) & np.uint32(0x7FFFFF)).astype(np.uint32)


@functools.lru_cache(None)
def div_triples():
    """(numerator, numerator, denominator) triples: the five pair families of tools/fastmath_exhaustive.hip, 2^19 triples
    (2^20 quotients) each, then special denominators and the structured set."""
    rng = np.random.default_rng(131)
    N = 1 << 19
    fam = []
    # 0: random bit patterns
    fam.append((rand_bits(rng, N), rand_bits(rng, N), rand_bits(rng, N)))
    # 1: exponents within +-40 of 1.0 (the perspective divide's range)
    fam.append(tuple(with_exp(rand_bits(rng, N), 87, 81) for _ in range(3)))
    # 2: structured mantissas under random signs and exponents
    fam.append(tuple((rand_bits(rng, N) & np.uint32(0xFF800000)) | structured_mants(rng, N) for _ in range(3)))
    # 3: a = RN(q * b) +- {0, 1, 2} ulps: quotients at and next to rounding boundaries
    ub, uq = with_exp(rand_bits(rng, N), 100, 55), with_exp(rand_bits(rng, N), 100, 55)
    ua = (u32(f32(uq) * f32(ub)).astype(np.int64) + rng.integers(-2, 3, N)).astype(np.uint32)
    fam.append((ua, ua ^ np.uint32(1), ub))
    # 4: numerators +-0, denormal, 2^-107, 2^-100, 2^123 against every ordinary denominator exponent
    r = rand_bits(rng, N) & np.uint32(0x807FFFFF)
    kinds = [np.uint32(0), SIGN, r, r | np.uint32(20 << 23), r | np.uint32(27 << 23), r | np.uint32(250 << 23)]
    ua = np.choose(rng.integers(0, 6, N), kinds).astype(np.uint32)
    fam.append((ua, ua ^ SIGN, with_exp(rand_bits(rng, N), 60, 135)))
    # denominators 0, +-inf, NaN, denormal (any denormal here, not only the tiny ones) under structured numerators
    M = 1 << 16
    core = structured_core()
    den = np.where(rng.integers(0, 2, M) == 0, div_bad_den(rng, M), (rand_bits(rng, M) & np.uint32(0x807FFFFF))).astype(np.uint32)
    fam.append((core[rng.integers(0, len(core), M)], rand_bits(rng, M), den))
    # the structured set in all three places
    rolls = (1, 17, 257, 1031, 2053, 3001, 4001, 4093)
    fam.append((np.tile(core, len(rolls)), np.tile(np.roll(core, 5), len(rolls)), np.concatenate([np.roll(core, k) for k in rolls])))
    out = tuple(np.concatenate([f[k] for f in fam]) for k in range(3))
    for o in out:
        o.setflags(write=False)
    return out


def zero_numerators(rng, interior, ncols):
    """Whole wavefronts of interior records in which about a third of the numerators are +0 or -0.  div_fast answers a zero
    numerator itself (q = a * y keeps the sign of -0, ok stays set), so nobody votes and the production function returns that."""
    q = interior[: 64 * MIXED_WAVES].copy()
    for k in range(ncols):
        hit = rng.integers(0, 3, len(q)) == 0
        q[hit, k] = np.where(rng.integers(0, 2, int(hit.sum())) == 0, np.uint32(0), SIGN)
    return q


@functools.lru_cache(None)
def div2_layout():
    rng = np.random.default_rng(141)
    a, b, c = div_triples()
    n = 64 * PURE_WAVES
    interior = records(div_interior(rng, n), div_interior(rng, n), div_interior(rng, n))
    fallback = interior[:4098].copy()
    k = np.arange(4098)
    fallback[k % 3 == 0, 2] = div_bad_den(rng, int((k % 3 == 0).sum()))
    fallback[k % 3 == 1, 0] = tiny_num(rng, int((k % 3 == 1).sum()))
    fallback[k % 3 == 2, 1] = tiny_num(rng, int((k % 3 == 2).sum()))
    return Layout(records(a, b, c), interior, fallback, 142, quiet=zero_numerators(rng, interior, 2))


@functools.lru_cache(None)
def div3_layout():
    rng = np.random.default_rng(151)
    a, b, c = div_triples()
    n = 64 * PURE_WAVES
    interior = records(div_interior(rng, n), div_interior(rng, n), div_interior(rng, n), div_interior(rng, n))
    fallback = interior[:4096].copy()
    k = np.arange(4096)
    fallback[k % 4 == 3, 3] = div_bad_den(rng, int((k % 4 == 3).sum()))
    for j in range(3):
        fallback[k % 4 == j, j] = tiny_num(rng, int((k % 4 == j).sum()))
    return Layout(records(a, b, np.roll(a, 3), c), interior, fallback, 152, quiet=zero_numerators(rng, interior, 3))


@functools.lru_cache(None)
def div2_reference():
    r = div2_layout().records
    return ref_div(f32(r[:, 0]), f32(r[:, 2])), ref_div(f32(r[:, 1]), f32(r[:, 2]))


# ---- rt_fastmath.h: the production functions, every wavefront composition ---------------------------
def test_rcp(tracer):
    """rtf::rcp(x) == RN(1 / x) for pure, mixed and ragged wavefronts.  The test checks VALUES, not control flow: replacing the
    ballot by a per-lane `if (!ok)` keeps it green, since both compute the same numbers; what it pins is that every lane gets
    the correctly rounded value whichever path its wavefront takes."""
    lay = rcp_layout()
    check_sections(tracer, "rcp", lay, {0: ref_rcp(f32(lay.records[:, 0]))})


def test_rcp3(tracer):
    """rtf::rcp3: three reciprocals behind one vote; a fallback operand in any of the three sends all three to IEEE."""
    lay = rcp3_layout()
    check_sections(tracer, "rcp3", lay, {k: ref_rcp(f32(lay.records[:, k])) for k in range(3)})


def test_sqrt(tracer):
    lay = sqrt_layout()
    check_sections(tracer, "sqrt", lay, {0: ref_sqrt(f32(lay.records[:, 0]))})


def test_rcp_sqrt(tracer):
    """rtf::rcp_sqrt(x) == RN(1 / RN(sqrt x)), both roundings."""
    lay = sqrt_layout()
    check_sections(tracer, "rcp_sqrt", lay, {0: ref_rcp_sqrt(f32(lay.records[:, 0]))})


def test_div2(tracer):
    """rtf::div2: two quotients that share a reciprocal, on the five pair families of tools/fastmath_exhaustive.hip."""
    q0, q1 = div2_reference()
    check_sections(tracer, "div2", div2_layout(), {0: q0, 1: q1})


def test_div3(tracer):
    lay = div3_layout()
    r = lay.records
    check_sections(tracer, "div3", lay, {k: ref_div(f32(r[:, k]), f32(r[:, 3])) for k in range(3)})


# ---- rt_fastmath.h: the fast paths' own values and guards --------------------------------------------
def fast_case(name):
    """(op, layout, reference of the fast value, word of the fast value, word of ok)."""
    if name == "rcp":
        lay = rcp_layout()
        return "rcp", lay, ref_rcp(f32(lay.records[:, 0])), 1, 2
    if name == "sqrt":
        lay = sqrt_layout()
        return "sqrt", lay, ref_sqrt(f32(lay.records[:, 0])), 1, 2
    if name == "rcp_sqrt":
        lay = sqrt_layout()
        return "rcp_sqrt", lay, ref_rcp_sqrt(f32(lay.records[:, 0])), 1, 2
    return "div2", div2_layout(), div2_reference()[0], 2, 3


@pytest.mark.parametrize("name", ["rcp", "sqrt", "rcp_sqrt", "div"])
def test_fast_path_guards(tracer, name):
    """The *_fast functions and their `ok` flags, lane by lane (they do not depend on the neighbours).
    ok implies the fast value is the correctly rounded one: a guard that is too loose fails here.
    ok holds on every interior operand: a guard that never fires (a silent loss of the fast path) fails here.
    The operands the mixed sections plant as fallback-needing do clear ok: otherwise those sections would test nothing.
    sqrt_fast / rcp_sqrt_fast: ok == (2^-100 <= x < inf) exactly, as the code states."""
    op, lay, want, vcol, okcol = fast_case(name)
    got = tracer.device_math(op, lay.records)
    ok = got[:, okcol]
    assert ((ok == 0) | (ok == 1)).all(), f"{op}: ok is neither 0 nor 1"
    ok = ok == 1
    check(got[ok, vcol], want[ok], f"{op}: fast value where ok is set", lay.records[ok])
    missed = lay.interior & ~ok
    assert not missed.any(), f"{op}: ok is clear on {int(missed.sum())} interior operands, e.g. {lay.records[missed][:4].tolist()}"
    voted = lay.fallback & ok
    if name == "div":       # word 3 is the guard of a / c alone: a record whose planted operand is the OTHER numerator keeps it set
        bexp = (lay.records[:, 1] >> np.uint32(23)) & np.uint32(0xFF)
        voted &= (bexp >= 87) & (bexp <= 167)
    assert not voted.any(), f"{op}: {int(voted.sum())} planted fallback operands keep ok set, e.g. {lay.records[voted][:4].tolist()}"
    assert 0 < int(ok.sum()) < len(ok)
    if name == "div":       # zero numerators keep ok set: that section of test_div2 really runs the fast path
        assert ok[lay.quiet].all(), "div_fast: ok is clear on a zero numerator over an ordinary denominator"
    if name in ("sqrt", "rcp_sqrt"):
        x = f32(lay.records[:, 0])
        with np.errstate(invalid="ignore"):
            expect = (x >= np.float32(2.0 ** -100)) & (x < np.float32(np.inf))
        assert (ok == expect).all(), f"{op}: ok != (2^-100 <= x < inf) on {int((ok != expect).sum())} operands"


# ---- rt_mesa_math.h, device instantiation --------------------------------------------------------
def mesa_device(tracer, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return tracer.device_math("mesa", records(u32(x)))


def test_mesa_device_vs_llvmpipe(tracer):
    """sin, cos, tan, exp on the device against the llvmpipe fixture, with test_mesa_trig_host's masks: |x| < 1.6e9 or
    non-finite for sin / cos / tan (the documented range of rtm::sincos), every input for exp."""
    g = load_golden("trig")
    x, ref = g["trig_in"], g["trig_out"]
    got = mesa_device(tracer, x)
    ok = (np.abs(x) < 1.6e9) | ~np.isfinite(x)
    assert ok.sum() > 0
    for k, name in enumerate(("sin", "cos", "tan")):
        check(got[ok, k], np.ascontiguousarray(ref[ok, k], dtype=np.float32), f"device {name} vs llvmpipe", u32(x)[ok])
    y, refe = g["explog_in"], np.ascontiguousarray(g["explog_out"][:, 3], dtype=np.float32)
    check(mesa_device(tracer, y)[:, 3], refe, "device exp vs llvmpipe", u32(np.ascontiguousarray(y, dtype=np.float32)))
    half = (g["fov_in"] * np.float32(0.017453292519943295)) * np.float32(0.5)
    check(mesa_device(tracer, half)[:, 2], np.ascontiguousarray(g["fov_tan"], dtype=np.float32), "device tan(radians(fov) / 2)")


@functools.lru_cache(None)
def mesa_wide_inputs():
    log2e = np.float32(1.44269504088896340736)
    k = np.float32(2.0 ** 31 * np.pi / 4)              # where (int32_t)(x * 4/pi) leaves int32
    parts = [structured_bits()]
    parts += [near(v, 64) for v in (k, k * np.float32(2), k * np.float32(0.5), np.float32(1.6e9), np.float32(2.0 ** 31), np.float32(2.0 ** 32))]
    parts.append(u32(np.array([1e10, 1e20, 3e38, -1e10, -1e20, -3e38], dtype=np.float32)))
    oct_ = (np.arange(0, 4097, dtype=np.float64) * (np.pi / 4)).astype(np.float32)       # octant boundaries, +-1 ulp
    ob = u32(oct_)
    parts += [ob, ob + np.uint32(1), np.maximum(ob, 1) - np.uint32(1), ob | SIGN]
    lo, hi = np.float32(-126.99999) / log2e, np.float32(128.0) / log2e      # exp's clamp points
    parts += [near(v, 64) for v in (lo, hi, np.float32(-87.33655), np.float32(-103.9721), np.float32(88.72284), np.float32(1.0))]
    out = np.concatenate(parts)
    out.setflags(write=False)
    return out


def test_mesa_device_vs_host(tracer, host):
    """Device against host instantiation of rt_mesa_math.h (the one pinned to llvmpipe by test_mesa_trig_host), bit for bit,
    NO mask: every exponent, +-0, denormals, +-inf, NaN, arguments up to and beyond 2^31 * pi/4 (the cvttps2dq guard), exp
    across both clamp points.  What may lower differently: (int32_t)y, fminf / fmaxf on NaN, floorf, tan's division, the
    shift that builds 2^ip."""
    bits = mesa_wide_inputs()
    x = f32(bits)
    want = host.mesa_math(x)
    assert want.dtype == np.float32 and want.shape == (len(x), 4)
    got = tracer.device_math("mesa", records(bits))
    for k, name in enumerate(("sin", "cos", "tan", "exp")):
        check(got[:, k], np.ascontiguousarray(want[:, k]), f"device {name} vs host", bits)


# ---- helpers of rt_kernels.hip ---------------------------------------------------------------------
# the edge list of tests/test_bloom.py::test_bloom_hip_bit_exact_vs_oracle
BLOOM_EDGES = np.array([0.0, 2.0 ** -25, 2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -24 * 1023.9, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12),
                        6.1e-5, 1.0 / 3.0, 0.1, 1.0009765, 1.00146, 65504.0, 65519.9, 65520.0, 65536.0, 1e5, 3e38, 1e-30, 1e-40],
                       dtype=np.float32)


@functools.lru_cache(None)
def f2h_inputs():
    h = np.arange(1 << 16, dtype=np.uint32)
    sel = np.isin((h >> 10) & 31, (0, 1, 14, 15, 30, 31))
    hv = u32(h[sel].astype(np.uint16).view(np.float16).astype(np.float32))      # every such half, exactly, as a float
    out = np.concatenate([structured_bits(), u32(BLOOM_EDGES), u32(-BLOOM_EDGES), hv, hv + np.uint32(1), hv - np.uint32(1)])
    out.setflags(write=False)
    return out


def test_f2h_rtz(tracer, oracle):
    """f2h_rtz (gNormal's store: fp32 -> fp16 toward zero) against the oracle's conversion: the fp16 denormal range, both ends
    of the normal range, saturation, inf and NaN, one ulp either side of the halfs where the code changes path."""
    bits = f2h_inputs()
    want = oracle.float_to_half_rtz(f32(bits)).astype(np.uint32)
    got = tracer.device_math("f2h", records(bits))[:, 0]
    assert (got >> 16 == 0).all(), "f2h_rtz set bits above the half"
    eq = (got == want) | (((got & 0x7FFF) > 0x7C00) & ((want & 0x7FFF) > 0x7C00))       # any half NaN equals any half NaN
    bad = np.flatnonzero(~eq)
    assert not len(bad), f"f2h_rtz: {len(bad)} differ, e.g. " + ", ".join(
        f"{int(bits[i]):08x} -> {int(got[i]):04x} want {int(want[i]):04x}" for i in bad[:8])
    # independent of the oracle's code: the result never exceeds the input in magnitude and is less than one half-ulp below
    fin = np.isfinite(f32(bits)) & (np.abs(f32(bits)) < 65536.0)
    back = got[fin].astype(np.uint16).view(np.float16).astype(np.float64)
    src = f32(bits)[fin].astype(np.float64)
    up = ((got[fin] & 0x7FFF) + 1).astype(np.uint16).view(np.float16).astype(np.float64)     # next half away from zero (inf at the top)
    assert (np.abs(back) <= np.abs(src)).all() and (np.abs(src) < np.abs(up)).all() and (np.signbit(back) == np.signbit(src)).all()


def test_half_bits_to_float(tracer):
    """All 2^16 half patterns against numpy's float16 -> float32 conversion; the words' high halves are noise."""
    h = np.arange(1 << 16, dtype=np.uint32)
    noise = rand_bits(np.random.default_rng(9), 1 << 16) << np.uint32(16)
    got = tracer.device_math("f2h", records(np.zeros(1 << 16, np.uint32), h | noise))[:, 1]
    want = h.astype(np.uint16).view(np.float16).astype(np.float32)
    check(got, want, "half_bits_to_float", h)


def test_pow5(tracer):
    """pow5(x) == ((x*x)*(x*x))*x in float32, NaN for x < 0, -0 in gives -0 out."""
    rng = np.random.default_rng(17)
    bits = np.concatenate([structured_bits(), u32(rng.uniform(-2.0, 2.0, 1 << 18).astype(np.float32))])
    assert_host_keeps_denormals()
    x = f32(bits)
    with np.errstate(all="ignore"):
        x2 = x * x
        want = np.where(x < 0, np.float32(np.nan), (x2 * x2) * x).astype(np.float32)
    assert u32(want[bits == SIGN])[0] == SIGN       # -0 -> -0
    check(tracer.device_math("pow5", records(bits))[:, 0], want, "pow5", bits)


def test_halton_eval(tracer, oracle):
    """halton_eval against the oracle's haltonSequence: bases 2, 3, 5, 7; indices 0 .. 4095 and 2^k - 1, 2^k, 3^k up to int32."""
    idx = list(range(4096)) + [2 ** k - 1 for k in range(32)] + [2 ** k for k in range(31)] + [3 ** k for k in range(20)]
    assert max(idx) == 2 ** 31 - 1
    idx = np.array(idx, dtype=np.int32)
    index = np.tile(idx, 4)
    base = np.repeat(np.array([2, 3, 5, 7], dtype=np.int32), len(idx))
    want = oracle.halton(index, base)
    got = tracer.device_math("halton", records(index.view(np.uint32), base.view(np.uint32)))
    check(got[:, 0], want, "halton_eval", np.stack([index, base], axis=1).view(np.uint32))
    assert (got[:, 1:] == 0).all()


# ---- the entry itself ----------------------------------------------------------------------------
def test_device_math_arguments(tracer, host):
    """With a live context: unknown ops, NULL and misaligned pointers are refused, n == 0 is a no-op that touches nothing, and
    a base < 2 gives HALTON's documented 0 instead of a loop that never ends."""
    import torch
    lib, ctx = tracer.lib, tracer.ctx
    d = torch.full((64, 4), 0x3F800000, dtype=torch.int32, device="cuda")
    o = torch.full((64, 4), 7, dtype=torch.int32, device="cuda")
    dp, op_ = ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(o.data_ptr())
    for bad_op in (-1, len(host.DEVICE_MATH_OPS), 1 << 20):
        assert lib.rt_debug_device_math(ctx, bad_op, dp, op_, 64, None) == -1
    assert lib.rt_debug_device_math(ctx, 0, None, op_, 64, None) == -1
    assert lib.rt_debug_device_math(ctx, 0, dp, None, 64, None) == -1
    assert lib.rt_debug_device_math(ctx, 0, ctypes.c_void_p(d.data_ptr() + 4), op_, 1, None) == -1
    assert lib.rt_debug_device_math(ctx, 0, dp, ctypes.c_void_p(o.data_ptr() + 8), 1, None) == -1
    assert b"aligned" in lib.rt_last_error(ctx)
    assert lib.rt_debug_device_math(ctx, 0, dp, op_, 0, None) == 0
    assert lib.rt_debug_device_math(ctx, 0, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == 7).all(), "a refused or empty call wrote to the output"
    assert sorted(host.DEVICE_MATH_OPS.values()) == list(range(10))
    assert tracer.device_math("rcp", np.zeros((0, 4), np.uint32)).shape == (0, 4)
    got = tracer.device_math("halton", records(np.array([5, 5, 5], np.uint32), np.array([0, 1, 0xFFFFFFFF], np.uint32)))
    assert (got == 0).all()
    one = tracer.device_math("rcp", records(np.array([0x40000000], np.uint32)))        # a single lane: 1 / 2
    assert one.tolist() == [[0x3F000000, 0x3F000000, 1, 0]]
