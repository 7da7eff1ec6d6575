"""CPU tier: the rounding error of every route of accuracy_cases.py under emulation, against a float64 transform of the same input.

Every case the emulator plans on the route its table names (others skip by route, as test_emu_exec_contract.py does; the cases too long for
emulation are left to the GPU tier: Case.emu).  The emulation evaluates the phase factors of kern_trig.hpp and kern_lines.hpp exactly where
the GPU calls sincospif, and contracts into FMAs differently: the GPU tier (test_gpu_accuracy.py) is the one that measures the product.
The references of accuracy_cases.py are checked here against the oracle's own O(N^2) sums."""
import numpy as np
import pytest

import accuracy_cases as acc
import emu_harness as emu
import exec_contract_cases as t

EMU_CASES = [c for c in acc.CASES if c.emu]
TRIG_TYPES = ("dct1", "dct2", "dct3", "dct4", "dst1", "dst2", "dst3", "dst4")


@pytest.mark.parametrize("direction", ["forward", "inverse"])
@pytest.mark.parametrize("typ", TRIG_TYPES)
def test_trig_reference_is_the_oracles_sum(oracle, typ, direction):
    """the FFT-of-the-extension references of all eight kinds, both directions, against oracle.trig1d_ref (f64 sums rounded to f32 once)"""
    for n in (2, 3, 8, 17, 30, 64):
        x = oracle.random_real_batch(n, 3, 0x7B00 + n)
        got = acc.trig1d_exact(x, oracle.trig_kind(typ, direction))
        want = np.stack([oracle.trig1d_ref(x[b], n, typ, direction) for b in range(3)]).astype(np.float64)
        # one f32 rounding of the oracle's result (2^-24 relative) and the f64 noise of either side's n-term sum
        bound = 2.0 ** -24 * np.abs(want) + 1e-12 * n
        assert np.all(np.abs(got - want) <= bound), (typ, direction, n, float(np.max(np.abs(got - want))))
    opts = t._o(typ, [30], 3, direction, "backward", layout=dict(t.REAL))
    x = oracle.random_real_batch(30, 3, 0x7B77).reshape(-1)
    want = oracle.trig_ref_batch(x, [30], 3, typ, direction, "backward").astype(np.float64)
    got = acc.exact_trig(oracle, opts, x)
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want) + 1e-10)


@pytest.mark.parametrize("shape", [[6, 5], [8, 3, 4]])
@pytest.mark.parametrize("typ", TRIG_TYPES)
def test_nd_trig_reference_is_the_oracles(oracle, typ, shape):
    """exact_trig of rank > 1 (trig1d_exact along every axis) against oracle.trig_ref_batch, which stores f32 after every axis: each of the
    rank stores adds at most 2^-24 of the array's rms, amplified by no more than 2 by the later axes (the types I - III are no isometries)"""
    for direction, normalize in (("forward", "unitary"), ("inverse", "backward")):
        opts = t._o(typ, shape, 3, direction, normalize, layout=dict(t.REAL))
        x = oracle.random_real_batch(int(np.prod(shape)), 3, 0x7B80 + len(shape)).reshape(-1)
        want = oracle.trig_ref_batch(x, shape, 3, typ, direction, normalize).astype(np.float64)
        got = acc.exact_trig(oracle, opts, x)
        assert float(oracle.rel_l2(got, want)) <= 2 * len(shape) * 2.0 ** -24, (typ, shape, direction)


@pytest.mark.parametrize("shape", [[6, 5], [8, 3, 4], [7, 4]])
def test_nd_c2r_reference_is_the_oracles(oracle, shape):
    """exact_c2r of rank > 1 against the oracle's full complex inverse (fftnd_ref) of the Hermitian extension of the same packed spectrum,
    and the rank-general _in_spectrum against the signal it was made from.  Bars: the O(N^2) f32 oracle's own error (below 2^-20 at
    these sizes); the f32 rounding of the spectrum (2^-24 a bin, a unitary map) for the round trip"""
    batch, n, p = 2, int(np.prod(shape)), shape[0] // 2 + 1
    opts = t._o("c2r", shape, batch, "inverse", "backward")
    x, _ = acc._in_spectrum(0x7B90)(oracle, opts)
    got = acc.exact_c2r(opts, x).reshape(batch, n)
    sig = oracle.random_real_batch(n, batch, 0x7B90).astype(np.float64)
    assert float(oracle.rel_l2(got * np.sqrt(n), sig)) <= 2.0 ** -23
    spec = acc._cplx(x, batch, [p] + shape[1:])
    mirror = spec[np.ix_(np.arange(batch), *((-np.arange(s)) % s for s in reversed(shape[1:])), np.arange(p))]      # X[k0, -k1, -k2]
    full = np.zeros((batch, *reversed(shape)), np.complex128)
    full[..., :p] = spec
    for k0 in range(p, shape[0]):
        full[..., k0] = np.conj(mirror[..., shape[0] - k0])
    for b in range(batch):
        ref = oracle.fftnd_ref(acc._inter(full[b]).astype(np.float32).reshape(-1), shape, "inverse", "backward", anysize=True).reshape(-1, 2)
        assert float(oracle.rel_l2(got[b], ref[:, 0].astype(np.float64))) <= 2.0 ** -20, (shape, b)


def test_view_and_fftconv_references_are_the_tables_oracles(oracle):
    """the float64 restatements of ioView / zeroPad and of fftconv (modes, boundaries, layouts) agree with the f32 oracles of
    exec_contract_cases.py on the same inputs, element for element, at the parity bar; the untouched elements are the same ones"""
    for name in ("lines_columns_mapped", "lines_c2r_mapped4096", "lines_mul_mapped100", "fftconv_nd_circular", "rconv_rank2", "rconv_widened1001",
                 "columns_ragged_r2c_64x64x8", "fftconv_fused64", "mixed_ct1000", "r2c_odd21", "xcd_fused_view_2p17", "fftconv_padded_domain"):
        case = acc.BY_NAME[name]
        _, _, want32, keep32 = t.data(oracle, case)
        _, _, want, keep = acc.data(oracle, case)
        assert np.array_equal(keep, keep32), name
        scale = float(np.max(np.abs(want[~keep])))
        assert np.max(np.abs(want[~keep] - want32[~keep])) <= 1e-5 * scale, name


def test_yardstick_is_guarded(oracle):
    """y(P) sits at 0.43 - 0.48 of 2^-24 sqrt(log2 P) (a radix-2 FFT with an f32 store per butterfly); acc.y itself refuses more than 0.5"""
    for lg in (3, 6, 10, 16):
        v = acc.y(oracle, 1 << lg) / (acc.U * np.sqrt(lg))
        assert 0.3 <= v <= 0.5, (lg, v)


@pytest.mark.parametrize("case", EMU_CASES, ids=repr)
def test_accuracy(oracle, monkeypatch, case):
    for k, v in case.emu_env.items():
        monkeypatch.setenv("MI355_EMU_" + k, v)
    desc, _ = t.desc_of(case.opts)
    route, _ = emu.route_of(desc)
    if not case.route_ok(route):
        pytest.skip(f"the emulator plans this request as {route.strip()}")
    x, kern, want, keep = acc.data(oracle, case)
    init = np.full(want.size, np.nan, np.float32) if keep.any() else None
    got, ran, _ = emu.run_plan(desc, x, want.size, kernel=kern, out_init=init)
    assert ran == route
    acc.measure(oracle, case, route, got[:want.size], want, keep)
