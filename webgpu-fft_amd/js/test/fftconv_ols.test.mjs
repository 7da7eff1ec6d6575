// GPU tier: the overlap-save route of real fftconv (lines-rconv-ols[N=P,L=L]: long real lines, short kernels, 1 + K launches) through the
// JavaScript host -> N-API addon -> C ABI.  Run by tests/test_js_fftconv_ols.py.  One request on the planner's own rule against a direct
// sum in float64 computed here; plan._route and plan._launchesPerExec show the route.
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

test("lines-rconv-ols: 20000 (*) 65 linear-same convolution, K = 2, the planner's own rule", async () => {
  const n = 20000, kn = 65, batch = 3, K = 2, off = (kn - 1) >> 1;
  const x = randomReal(n * batch, 31), h = randomReal(kn * K, 32);
  const opts = { type: "fftconv", shape: [n], batch, layout: REAL, fftConv: { mode: "convolution", boundary: "linear-same", kernelCount: K, kernelShape: [kn] } };
  const dev = await ensureDevice();
  const inBuf = dev.createBuffer({ size: x.byteLength, usage: usage() });
  dev.queue.writeBuffer(inBuf, 0, x);
  const outFloats = K * batch * n;
  const outBuf = dev.createBuffer({ size: outFloats * 4, usage: usage() });
  const plan = fft.createPlan(dev, opts);
  assert(/lines-r2c-mapped\[N=\d+\] lines-rconv-ols\[N=\d+,L=\d+\]/.test(plan._route) && plan._launchesPerExec === 1 + K, "route " + plan._route + " launches " + plan._launchesPerExec);
  const enc = dev.createCommandEncoder();
  plan.exec(enc, { input: inBuf, output: outBuf, kernel: h });
  dev.queue.submit([enc.finish()]);
  await dev.queue.onSubmittedWorkDone();
  await outBuf.mapAsync(GPUMapMode.READ, 0, outFloats * 4);
  const got = new Float32Array(outBuf.getMappedRange(0, outFloats * 4).slice(0));
  outBuf.unmap();
  let num = 0, den = 0;
  for (let k = 0; k < K; k++) for (let b = 0; b < batch; b++) for (let m = 0; m < n; m++) {      // kernel-major
    let acc = 0;
    for (let j = 0; j < kn; j++) { const p = m + off - j; if (p >= 0 && p < n) acc += x[b * n + p] * h[k * kn + j]; }
    const g = got[(k * batch + b) * n + m], d = g - acc;
    num += d * d; den += acc * acc;
    assert(Math.abs(d) <= 4e-3 + 4e-3 * Math.abs(acc), "kernel " + k + " line " + b + " element " + m + " got " + g + " want " + acc);
  }
  const l2 = Math.sqrt(num / den);
  console.log("       " + plan._route.trim() + ": rel_l2=" + l2.toExponential(3));
  assert(l2 < 1e-5, "rel_l2 " + l2);
  plan.destroy(); inBuf.destroy(); outBuf.destroy();
});

run();
