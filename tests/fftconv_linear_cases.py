"""Shared by test_emu_fftconv_linear.py and test_gpu_fftconv_linear.py: the long rank-1 fftconv requests of the padded-domain /
pipeline-view routes and their float64 reference.

The reference is computed at the EXACT logical FFT length fN = shape + kernelShape - 1 (circular: shape) with numpy's float64 FFT,
so it does not depend on the padding under test: y = ifft(fft(x, fN) * H), H = fft(k, fN) or its conjugate (correlation);
zeroPad.read is applied to x before the transform, zeroPad.write to the logical result before the crop."""
import numpy as np

FORBIDDEN_IN_PIPELINE_ROUTE = ("bluestein", "stages", "mixed", "gather", "scatter", "zero-read", "zero-write")

# shape, kernelShape, boundary, mode, K, layout, zeroPad  (the table of the pipeline-view route: FFT domain 2^20)
PIPELINE_CASES = {
    "full_conv_exact_2p20": (600000, 448577, "linear-full", "convolution", 1, "kernel-major", None),
    "same_conv_batch_major": (524288, 524288, "linear-same", "convolution", 2, "batch-major", None),
    "valid_corr_short_filter": (700000, 1000, "linear-valid", "correlation", 1, "kernel-major", None),
    "full_corr_wrapped_lags": (524288, 300000, "linear-full", "correlation", 2, "kernel-major", None),
    "circular_zero_pad": (1048576, 1000, "circular", "convolution", 1, "kernel-major",
                          {"read": {"start": [5], "end": [1000000]}, "write": {"start": [7], "end": [900001]}}),
    "same_corr_zero_write": (524288, 524288, "linear-same", "correlation", 1, "batch-major", {"write": {"start": [100000], "end": [400000]}}),
}
# the composed route on a padded domain other than 2^20
COMPOSED_CASES = {
    "full_corr_32999": (20000, 13000, "linear-full", "correlation", 2, "kernel-major", None),       # -> 65536
    "same_conv_69999": (40000, 30000, "linear-same", "convolution", 1, "kernel-major", None),        # -> 131072
    "valid_conv_1999999": (1400000, 600000, "linear-valid", "convolution", 1, "kernel-major", None),  # -> 2^21
}


def options(case, batch):
    n, kn, boundary, mode, K, layout, zero_pad = case
    opts = {"type": "fftconv", "shape": [n], "batch": batch,
            "fftConv": {"mode": mode, "boundary": boundary, "kernelCount": K, "kernelShape": [kn], "outputLayout": layout}}
    if zero_pad:
        opts["zeroPad"] = zero_pad
    return opts


def geometry(case):
    """(logical FFT length, output length, output offset on the logical domain)"""
    n, kn, boundary = case[0], case[1], case[2]
    if boundary == "circular":
        return n, n, 0
    fn = n + kn - 1
    if boundary == "linear-full":
        return fn, fn, 0
    if boundary == "linear-same":
        return fn, n, (kn - 1) // 2
    return fn, n - kn + 1, kn - 1


def reference(case, x, kern, lines):
    """float64 reference of the first `lines` data lines: float64 interleaved array [K][lines][os][2]"""
    n, kn, boundary, mode, K, layout, zero_pad = case
    fn, on, off = geometry(case)
    xc = np.asarray(x[:2 * n * lines], np.float64).reshape(lines, n, 2)
    xc = xc[..., 0] + 1j * xc[..., 1]
    if zero_pad and zero_pad.get("read"):
        keep = np.zeros(n, bool)
        keep[zero_pad["read"]["start"][0]:min(zero_pad["read"]["end"][0], n)] = True
        xc = np.where(keep, xc, 0)
    X = np.fft.fft(xc, fn, axis=-1)
    want = np.empty((K, lines, on, 2), np.float64)
    for k in range(K):
        kc = np.asarray(kern[2 * k * kn:2 * (k + 1) * kn], np.float64).reshape(kn, 2)
        H = np.fft.fft(kc[:, 0] + 1j * kc[:, 1], fn)
        y = np.fft.ifft(X * (np.conj(H) if mode == "correlation" else H), axis=-1)
        if zero_pad and zero_pad.get("write"):
            keep = np.zeros(fn, bool)
            keep[zero_pad["write"]["start"][0]:zero_pad["write"]["end"][0]] = True
            y = np.where(keep, y, 0)
        y = y[:, off:off + on]
        want[k, :, :, 0], want[k, :, :, 1] = y.real, y.imag
    return want


def kernel_major(got, case, batch):
    """the plan's output as [K][batch][os * 2] whatever its layout"""
    K, layout = case[4], case[5]
    on = geometry(case)[1]
    g = np.asarray(got)
    return g.reshape(K, batch, 2 * on) if layout == "kernel-major" else g.reshape(batch, K, 2 * on).transpose(1, 0, 2)


def reference_pow2(oracle, case, x, kern, lines):
    """the same through the oracle's fftConvRef restatement (use_pow2: its radix-2 path), for logical FFT lengths that are a power of two"""
    n, kn, boundary, mode, K, layout, zero_pad = case
    fn, on, off = geometry(case)
    assert fn & (fn - 1) == 0
    xin = np.array(x[:2 * n * lines], np.float32).reshape(lines, n, 2)
    if zero_pad and zero_pad.get("read"):
        keep = np.zeros(n, bool)
        keep[zero_pad["read"]["start"][0]:min(zero_pad["read"]["end"][0], n)] = True
        xin[:, ~keep] = 0
    want = np.empty((K, lines, on, 2), np.float64)
    for k in range(K):
        y, _ = oracle.fftconv_ref(xin.reshape(-1), kern[2 * k * kn:2 * (k + 1) * kn], [n], lines, mode, boundary, [kn], use_pow2=True)
        want[k] = np.asarray(y, np.float64).reshape(lines, on, 2)
    if zero_pad and zero_pad.get("write"):      # output coordinate o is logical coordinate o + off
        keep = np.zeros(on, bool)
        keep[max(0, zero_pad["write"]["start"][0] - off):max(0, min(on, zero_pad["write"]["end"][0] - off))] = True
        want[:, :, ~keep] = 0
    return want


def want_for(oracle, case, x, kern, lines):
    fn = geometry(case)[0]
    return reference_pow2(oracle, case, x, kern, lines) if fn & (fn - 1) == 0 else reference(case, x, kern, lines)
