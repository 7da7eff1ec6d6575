// GPU tier: the overlap-save tile route of rank-2 real fftconv (tiles-rconv-ols[N=PxP,L=L0xL1]: real images, small kernels, two real tiles as re / im of a
// complex one, 1 + K launches) through the JavaScript host -> N-API addon -> C ABI.  Run by tests/test_js_fftconv_rtiles.py.  Two requests against direct
// sums in float64 computed here; plan._route and plan._launchesPerExec show the route, getWorkspaceSizeBytes() the workspace of the K kernel spectra alone.
import { test, assert, run } from "./harness.mjs";
import * as fft from "../index.js";

let device = null;
async function ensureDevice() { if (!device) device = await fft.requestDevice(); return device; }
const usage = () => GPUBufferUsage.STORAGE | GPUBufferUsage.COPY_SRC | GPUBufferUsage.COPY_DST;

const REAL = { interleavedComplex: false };

function randomReal(n, seed) {
  const out = new Float32Array(n);
  let s = seed >>> 0;
  for (let i = 0; i < n; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; out[i] = s / 2147483648 - 1; }
  return out;
}

// linear-same, kernel-major: output o is index m = o + c of the logical domain of n + M - 1 points, c = floor((M - 1) / 2).  Convolution: y[m] = sum_r h[r] x[m - r].
// Correlation: y = sum_r h[r] x[lag + r], the lag m below n and m - (n + M - 1) from there on (the negative lags sit at the top of the domain)
async function check(name, n0, n1, m0, m1, batch, K, mode, P, tile) {
  const x = randomReal(n0 * n1 * batch, 61), h = randomReal(m0 * m1 * K, 62);
  const opts = { type: "fftconv", shape: [n0, n1], batch, layout: REAL, fftConv: { mode, boundary: "linear-same", kernelCount: K, kernelShape: [m0, m1] } };
  const dev = await ensureDevice();
  const inBuf = dev.createBuffer({ size: x.byteLength, usage: usage() });
  dev.queue.writeBuffer(inBuf, 0, x);
  const outFloats = K * batch * n0 * n1;
  const outBuf = dev.createBuffer({ size: outFloats * 4, usage: usage() });
  const saved = process.env.MI355FFT_RCONV_OLS2D;
  if (P) process.env.MI355FFT_RCONV_OLS2D = String(P);
  let plan;
  try { plan = fft.createPlan(dev, opts); } finally { if (P) { if (saved === undefined) delete process.env.MI355FFT_RCONV_OLS2D; else process.env.MI355FFT_RCONV_OLS2D = saved; } }
  const d = { route: plan._route, launchesPerExec: plan._launchesPerExec };
  const tag = "tiles-rspectrum[N=" + tile + "x" + tile + "] tiles-rconv-ols[N=" + tile + "x" + tile + ",L=" + (tile - m0 + 1) + "x" + (tile - m1 + 1) + "]";
  assert(d.route.includes(tag) && d.launchesPerExec === 1 + K, "route " + d.route + " launches " + d.launchesPerExec);
  const work = plan.getWorkspaceSizeBytes();
  assert(work >= K * tile * tile * 8 && work < (1 << 20), "workspace " + work);
  const enc = dev.createCommandEncoder();
  plan.exec(enc, { input: inBuf, output: outBuf, kernel: h });
  dev.queue.submit([enc.finish()]);
  await dev.queue.onSubmittedWorkDone();
  await outBuf.mapAsync(GPUMapMode.READ, 0, outFloats * 4);
  const got = new Float32Array(outBuf.getMappedRange(0, outFloats * 4).slice(0));
  outBuf.unmap();
  const lag = (m, n, M) => (m < n ? m : m - (n + M - 1));
  const corr = mode === "correlation", c0 = (m0 - 1) >> 1, c1 = (m1 - 1) >> 1;
  let num = 0, den = 0;
  for (let k = 0; k < K; k++) for (let b = 0; b < batch; b++) for (let o1 = 0; o1 < n1; o1++) for (let o0 = 0; o0 < n0; o0++) {
    let re = 0;
    for (let r1 = 0; r1 < m1; r1++) {
      const p1 = corr ? lag(o1 + c1, n1, m1) + r1 : o1 + c1 - r1;
      if (p1 < 0 || p1 >= n1) continue;
      for (let r0 = 0; r0 < m0; r0++) {
        const p0 = corr ? lag(o0 + c0, n0, m0) + r0 : o0 + c0 - r0;
        if (p0 < 0 || p0 >= n0) continue;
        re += x[(b * n1 + p1) * n0 + p0] * h[(k * m1 + r1) * m0 + r0];
      }
    }
    const at = ((k * batch + b) * n1 + o1) * n0 + o0, dr = got[at] - re;
    num += dr * dr; den += re * re;
    assert(Math.abs(dr) <= 4e-3 + 4e-3 * Math.abs(re),
           name + " kernel " + k + " image " + b + " element " + o0 + "," + o1 + " got " + got[at] + " want " + re);
  }
  const l2 = Math.sqrt(num / den);
  console.log("       " + d.route.trim() + ": rel_l2=" + l2.toExponential(3));
  assert(l2 <= 1e-5, "rel_l2 " + l2);
  plan.destroy(); inBuf.destroy(); outBuf.destroy();
}

test("tiles-rconv-ols: 150 x 130 (*) 9 x 5 linear-same convolution, batch 3, the 64-point tile forced (nb1 = 3: a pair row without its partner)", async () => {
  await check("150x130", 150, 130, 9, 5, 3, 1, "convolution", 64, 64);
});

test("tiles-rconv-ols: 300 x 200 (*) 9 x 9 linear-same correlation, K = 2, the planner's own rule", async () => {
  await check("300x200", 300, 200, 9, 9, 1, 2, "correlation", 0, 64);
});

run();
