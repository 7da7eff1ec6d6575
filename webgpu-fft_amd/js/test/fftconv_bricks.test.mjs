// GPU tier: the overlap-save brick routes of rank-3 fftconv (bricks-conv-ols / bricks-rconv-ols[N=16x16x16,L=L0xL1xL2]: volumes, small kernels, 1 + K launches)
// through the JavaScript host -> N-API addon -> C ABI.  Run by tests/test_js_fftconv_bricks.py.  Complex and real requests against direct sums in float64
// computed here; plan._route and plan._launchesPerExec show the route, getWorkspaceSizeBytes() the workspace of the K kernel spectra alone.
import { test, assert, run } from "./harness.mjs";
import * as fft from "../index.js";

let device = null;
async function ensureDevice() { if (!device) device = await fft.requestDevice(); return device; }
const usage = () => GPUBufferUsage.STORAGE | GPUBufferUsage.COPY_SRC | GPUBufferUsage.COPY_DST;

function randomFloats(n, seed) {
  const out = new Float32Array(n);
  let s = seed >>> 0;
  for (let i = 0; i < n; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; out[i] = s / 2147483648 - 1; }
  return out;
}

// linear-same, kernel-major: output o is index m = o + c of the logical domain of n + M - 1 points, c = floor((M - 1) / 2).  Convolution: y[m] = sum_r h[r] x[m - r].
// Correlation: y = sum_r conj(h[r]) x[lag + r], the lag m below n and m - (n + M - 1) from there on (the negative lags sit at the top of the domain).
// `real`: f32 elements (w = 1 float an element), else interleaved complex (w = 2)
async function check(name, real, n, m, batch, K, mode, forced) {
  const w = real ? 1 : 2, P = 16;
  const nn = n[0] * n[1] * n[2], mm = m[0] * m[1] * m[2];
  const x = randomFloats(w * nn * batch, real ? 71 : 73), h = randomFloats(w * mm * K, real ? 72 : 74);
  const opts = { type: "fftconv", shape: n, batch, fftConv: { mode, boundary: "linear-same", kernelCount: K, kernelShape: m } };
  if (real) opts.layout = { interleavedComplex: false };
  const dev = await ensureDevice();
  const inBuf = dev.createBuffer({ size: x.byteLength, usage: usage() });
  dev.queue.writeBuffer(inBuf, 0, x);
  const outFloats = w * K * batch * nn;
  const outBuf = dev.createBuffer({ size: outFloats * 4, usage: usage() });
  const name_ = real ? "MI355FFT_RCONV_OLS3D" : "MI355FFT_CONV_OLS3D", saved = process.env[name_];
  if (forced) process.env[name_] = String(P);
  let plan;
  try { plan = fft.createPlan(dev, opts); } finally { if (forced) { if (saved === undefined) delete process.env[name_]; else process.env[name_] = saved; } }
  const d = { route: plan._route, launchesPerExec: plan._launchesPerExec };
  const r = real ? "r" : "";
  const tag = "bricks-" + r + "spectrum[N=16x16x16] bricks-" + r + "conv-ols[N=16x16x16,L=" + (P - m[0] + 1) + "x" + (P - m[1] + 1) + "x" + (P - m[2] + 1) + "]";
  assert(d.route.includes(tag) && d.launchesPerExec === 1 + K, "route " + d.route + " launches " + d.launchesPerExec);
  const work = plan.getWorkspaceSizeBytes();
  assert(work >= K * 32768 && work < (1 << 20), "workspace " + work);
  const enc = dev.createCommandEncoder();
  plan.exec(enc, { input: inBuf, output: outBuf, kernel: h });
  dev.queue.submit([enc.finish()]);
  await dev.queue.onSubmittedWorkDone();
  await outBuf.mapAsync(GPUMapMode.READ, 0, outFloats * 4);
  const got = new Float32Array(outBuf.getMappedRange(0, outFloats * 4).slice(0));
  outBuf.unmap();
  const lag = (q, len, M) => (q < len ? q : q - (len + M - 1));
  const corr = mode === "correlation", c = m.map((v) => (v - 1) >> 1);
  const src = (o, a, ra) => (corr ? lag(o + c[a], n[a], m[a]) + ra : o + c[a] - ra);
  let num = 0, den = 0;
  for (let k = 0; k < K; k++) for (let b = 0; b < batch; b++) for (let o2 = 0; o2 < n[2]; o2++) for (let o1 = 0; o1 < n[1]; o1++) for (let o0 = 0; o0 < n[0]; o0++) {
    let re = 0, im = 0;
    for (let r2 = 0; r2 < m[2]; r2++) {
      const p2 = src(o2, 2, r2);
      if (p2 < 0 || p2 >= n[2]) continue;
      for (let r1 = 0; r1 < m[1]; r1++) {
        const p1 = src(o1, 1, r1);
        if (p1 < 0 || p1 >= n[1]) continue;
        for (let r0 = 0; r0 < m[0]; r0++) {
          const p0 = src(o0, 0, r0);
          if (p0 < 0 || p0 >= n[0]) continue;
          const xa = w * (((b * n[2] + p2) * n[1] + p1) * n[0] + p0), ha = w * (((k * m[2] + r2) * m[1] + r1) * m[0] + r0);
          const xr = x[xa], xi = real ? 0 : x[xa + 1], hr = h[ha], hi = real ? 0 : (corr ? -h[ha + 1] : h[ha + 1]);
          re += xr * hr - xi * hi; im += xr * hi + xi * hr;
        }
      }
    }
    const at = w * ((((k * batch + b) * n[2] + o2) * n[1] + o1) * n[0] + o0), dr = got[at] - re, di = real ? 0 : got[at + 1] - im;
    num += dr * dr + di * di; den += re * re + im * im;
    assert(Math.abs(dr) <= 4e-3 + 4e-3 * Math.abs(re) && Math.abs(di) <= 4e-3 + 4e-3 * Math.abs(im),
           name + " kernel " + k + " volume " + b + " element " + o0 + "," + o1 + "," + o2 + " got " + got[at] + " want " + re + "," + im);
  }
  const l2 = Math.sqrt(num / den);
  console.log("       " + d.route.trim() + ": rel_l2=" + l2.toExponential(3));
  assert(l2 <= 1e-5, "rel_l2 " + l2);
  plan.destroy(); inBuf.destroy(); outBuf.destroy();
}

test("bricks-conv-ols: 30 x 20 x 18 (*) 5 x 3 x 4 linear-same convolution, batch 2, the brick forced", async () => {
  await check("30x20x18", false, [30, 20, 18], [5, 3, 4], 2, 1, "convolution", true);
});

test("bricks-rconv-ols: 30 x 20 x 18 (*) 5 x 3 x 4 linear-same convolution, batch 2, the brick forced (nb2 = 2: both partners)", async () => {
  await check("r30x20x18", true, [30, 20, 18], [5, 3, 4], 2, 1, "convolution", true);
});

test("bricks-conv-ols: 40 x 36 x 34 (*) 3 x 3 x 3 linear-same correlation, K = 2, the planner's own rule", async () => {
  await check("40x36x34", false, [40, 36, 34], [3, 3, 3], 1, 2, "correlation", false);
});

test("bricks-rconv-ols: 40 x 36 x 34 (*) 3 x 3 x 3 linear-same correlation, K = 2, the planner's own rule", async () => {
  await check("r40x36x34", true, [40, 36, 34], [3, 3, 3], 1, 2, "correlation", false);
});

run();
