// GPU tier: boundary "circular" on the overlap-save routes of fftconv (route tags ending in ",wrap]": a block's halo at the edge of the domain comes from the
// other end of the signal) through the JavaScript host -> N-API addon -> C ABI.  Run by tests/test_js_fftconv_circular.py.  One complex request (rank 2, tiles) and
// one real request (rank 1, an odd line) against direct circular sums in float64 computed here; plan._route and plan._launchesPerExec show the route, and
// with MI355FFT_OLS_CIRCULAR=0 the same request plans without the tag.
import { test, assert, run } from "./harness.mjs";
import * as fft from "../index.js";

let device = null;
async function ensureDevice() { if (!device) device = await fft.requestDevice(); return device; }
const usage = () => GPUBufferUsage.STORAGE | GPUBufferUsage.COPY_SRC | GPUBufferUsage.COPY_DST;

function random(n, seed) {
  const out = new Float32Array(n);
  let s = seed >>> 0;
  for (let i = 0; i < n; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; out[i] = s / 2147483648 - 1; }
  return out;
}
const mod = (a, n) => ((a % n) + n) % n;

function planAt(dev, opts, value) {
  const saved = process.env.MI355FFT_OLS_CIRCULAR;
  if (value !== null) process.env.MI355FFT_OLS_CIRCULAR = value;
  try { return fft.createPlan(dev, opts); } finally { if (saved === undefined) delete process.env.MI355FFT_OLS_CIRCULAR; else process.env.MI355FFT_OLS_CIRCULAR = saved; }
}

// circular, kernel-major.  Convolution: y[m] = sum_r h[r] x[(m - r) mod n].  Correlation: y[m] = sum_r conj(h[r]) x[(m + r) mod n].  W = 2: interleaved complex, W = 1: real
async function check(name, shape, ks, batch, K, mode, real, tag, spectrumBytes) {
  const W = real ? 1 : 2, [n0, n1] = [shape[0], shape[1] || 1], [m0, m1] = [ks[0], ks[1] || 1];
  const x = random(W * n0 * n1 * batch, 71), h = random(W * m0 * m1 * K, 72);
  const opts = { type: "fftconv", shape, batch, fftConv: { mode, boundary: "circular", kernelCount: K, kernelShape: ks } };
  if (real) opts.layout = { interleavedComplex: false };
  const dev = await ensureDevice();
  const old = planAt(dev, opts, "0");
  assert(!old._route.includes("wrap"), "route with the switch at 0: " + old._route);
  old.destroy();
  const plan = planAt(dev, opts, null);
  assert(plan._route.includes(tag) && plan._launchesPerExec === 1 + K, "route " + plan._route + " launches " + plan._launchesPerExec);
  const work = plan.getWorkspaceSizeBytes();
  assert(work >= K * spectrumBytes && work < K * spectrumBytes + 256, "workspace " + work);
  const inBuf = dev.createBuffer({ size: x.byteLength, usage: usage() });
  dev.queue.writeBuffer(inBuf, 0, x);
  const outFloats = W * K * batch * n0 * n1;
  const outBuf = dev.createBuffer({ size: outFloats * 4, usage: usage() });
  const enc = dev.createCommandEncoder();
  plan.exec(enc, { input: inBuf, output: outBuf, kernel: h });
  dev.queue.submit([enc.finish()]);
  await dev.queue.onSubmittedWorkDone();
  await outBuf.mapAsync(GPUMapMode.READ, 0, outFloats * 4);
  const got = new Float32Array(outBuf.getMappedRange(0, outFloats * 4).slice(0));
  outBuf.unmap();
  const corr = mode === "correlation";
  let num = 0, den = 0;
  for (let k = 0; k < K; k++) for (let b = 0; b < batch; b++) for (let o1 = 0; o1 < n1; o1++) for (let o0 = 0; o0 < n0; o0++) {
    let re = 0, im = 0;
    for (let r1 = 0; r1 < m1; r1++) {
      const p1 = mod(corr ? o1 + r1 : o1 - r1, n1);
      for (let r0 = 0; r0 < m0; r0++) {
        const p0 = mod(corr ? o0 + r0 : o0 - r0, n0);
        const xa = W * ((b * n1 + p1) * n0 + p0), ha = W * ((k * m1 + r1) * m0 + r0);
        const xr = x[xa], xi = real ? 0 : x[xa + 1], hr = h[ha], hi = real ? 0 : (corr ? -h[ha + 1] : h[ha + 1]);
        re += xr * hr - xi * hi; im += xr * hi + xi * hr;
      }
    }
    const at = W * (((k * batch + b) * n1 + o1) * n0 + o0), dr = got[at] - re, di = real ? 0 : got[at + 1] - im;
    num += dr * dr + di * di; den += re * re + im * im;
    assert(Math.abs(dr) <= 4e-3 + 4e-3 * Math.abs(re) && Math.abs(di) <= 4e-3 + 4e-3 * Math.abs(im),
           name + " kernel " + k + " item " + b + " element " + o0 + "," + o1 + " got " + got[at] + " want " + re + "," + im);
  }
  const l2 = Math.sqrt(num / den);
  console.log("       " + plan._route.trim() + ": rel_l2=" + l2.toExponential(3));
  assert(l2 <= 1e-5, "rel_l2 " + l2);
  plan.destroy(); inBuf.destroy(); outBuf.destroy();
}

test("tiles-conv-ols, wrap: complex 150 x 130 (*) 9 x 5 circular convolution, batch 2 (3 x 3 tiles: every edge tile wraps)", async () => {
  await check("150x130", [150, 130], [9, 5], 2, 1, "convolution", false, "tiles-spectrum[N=64x64] tiles-conv-ols[N=64x64,L=56x60,wrap]", 64 * 64 * 8);
});

test("lines-rconv-ols, wrap: real 8193 (*) 31 circular correlation, batch 2, K = 2 (an odd line: sample pairs across the seam)", async () => {
  await check("8193", [8193], [31], 2, 2, "correlation", true, "lines-r2c-mapped[N=1024] lines-rconv-ols[N=1024,L=994,wrap]", 513 * 8);
});

run();
