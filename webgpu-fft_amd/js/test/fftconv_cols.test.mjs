// GPU tier: the overlap-save route of complex fftconv (lines-conv-ols[N=P,L=L]: long complex lines, short kernels, 1 + K launches) through the
// JavaScript host -> N-API addon -> C ABI.  Run by tests/test_js_fftconv_cols.py.  One request on the planner's own rule against a direct
// sum in float64 computed here; plan._route and plan._launchesPerExec show the route, getWorkspaceSizeBytes() the workspace of the K kernel spectra alone.
import { test, assert, run } from "./harness.mjs";
import * as fft from "../index.js";

let device = null;
async function ensureDevice() { if (!device) device = await fft.requestDevice(); return device; }
const usage = () => GPUBufferUsage.STORAGE | GPUBufferUsage.COPY_SRC | GPUBufferUsage.COPY_DST;

function randomInterleaved(n, seed) {
  const out = new Float32Array(2 * n);
  let s = seed >>> 0;
  for (let i = 0; i < 2 * n; i++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; out[i] = s / 2147483648 - 1; }
  return out;
}

test("lines-conv-ols: 20000 (*) 65 linear-same convolution, K = 2, the planner's own rule", async () => {
  const n = 20000, kn = 65, batch = 3, K = 2, off = (kn - 1) >> 1;
  const x = randomInterleaved(n * batch, 41), h = randomInterleaved(kn * K, 42);
  const opts = { type: "fftconv", shape: [n], batch, fftConv: { mode: "convolution", boundary: "linear-same", kernelCount: K, kernelShape: [kn] } };
  const dev = await ensureDevice();
  const inBuf = dev.createBuffer({ size: x.byteLength, usage: usage() });
  dev.queue.writeBuffer(inBuf, 0, x);
  const outFloats = 2 * K * batch * n;
  const outBuf = dev.createBuffer({ size: outFloats * 4, usage: usage() });
  const plan = fft.createPlan(dev, opts);
  const d = { route: plan._route, launchesPerExec: plan._launchesPerExec };
  assert(/lines-mapped\[N=\d+\] lines-conv-ols\[N=\d+,L=\d+\]/.test(d.route) && d.launchesPerExec === 1 + K, "route " + d.route + " launches " + d.launchesPerExec);
  const work = plan.getWorkspaceSizeBytes();
  assert(work >= K * 1024 * 8 && work < (1 << 20), "workspace " + work);
  const enc = dev.createCommandEncoder();
  plan.exec(enc, { input: inBuf, output: outBuf, kernel: h });
  dev.queue.submit([enc.finish()]);
  await dev.queue.onSubmittedWorkDone();
  await outBuf.mapAsync(GPUMapMode.READ, 0, outFloats * 4);
  const got = new Float32Array(outBuf.getMappedRange(0, outFloats * 4).slice(0));
  outBuf.unmap();
  let num = 0, den = 0;
  for (let k = 0; k < K; k++) for (let b = 0; b < batch; b++) for (let m = 0; m < n; m++) {      // kernel-major
    let re = 0, im = 0;
    for (let j = 0; j < kn; j++) {
      const p = m + off - j;
      if (p < 0 || p >= n) continue;
      const xr = x[2 * (b * n + p)], xi = x[2 * (b * n + p) + 1], hr = h[2 * (k * kn + j)], hi = h[2 * (k * kn + j) + 1];
      re += xr * hr - xi * hi; im += xr * hi + xi * hr;
    }
    const at = 2 * ((k * batch + b) * n + m), dr = got[at] - re, di = got[at + 1] - im;
    num += dr * dr + di * di; den += re * re + im * im;
    assert(Math.abs(dr) <= 4e-3 + 4e-3 * Math.abs(re) && Math.abs(di) <= 4e-3 + 4e-3 * Math.abs(im),
           "kernel " + k + " line " + b + " element " + m + " got " + got[at] + "," + got[at + 1] + " want " + re + "," + im);
  }
  const l2 = Math.sqrt(num / den);
  console.log("       " + d.route.trim() + ": rel_l2=" + l2.toExponential(3));
  assert(l2 < 1e-5, "rel_l2 " + l2);
  plan.destroy(); inBuf.destroy(); outBuf.destroy();
});

run();
