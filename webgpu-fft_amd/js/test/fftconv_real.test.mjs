// GPU tier: fftconv over real data (type "fftconv" with layout.interleavedComplex false -> MI355FFT_FFTCONV_REAL) through the
// JavaScript host -> N-API addon -> C ABI.  Run by tests/test_js_fftconv_real.py.  Plan creation, one case on the one-launch line
// route (lines-rconv) and one on the composed route (rconv[K]), each against a direct sum in float64 computed here.
import { test, assert, assertThrows, run } from "./harness.mjs";
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

async function runPlan(opts, x, kernel, outFloats) {
  const dev = await ensureDevice();
  const inBuf = dev.createBuffer({ size: x.byteLength, usage: usage() });
  dev.queue.writeBuffer(inBuf, 0, x);
  const outBuf = dev.createBuffer({ size: outFloats * 4, usage: usage() });
  const plan = fft.createPlan(dev, opts);
  const enc = dev.createCommandEncoder();
  plan.exec(enc, { input: inBuf, output: outBuf, kernel });
  dev.queue.submit([enc.finish()]);
  await dev.queue.onSubmittedWorkDone();
  await outBuf.mapAsync(GPUMapMode.READ, 0, outFloats * 4);
  const out = new Float32Array(outBuf.getMappedRange(0, outFloats * 4).slice(0));
  outBuf.unmap();
  const r = { out, route: plan._route, launches: plan._launchesPerExec };
  plan.destroy(); inBuf.destroy(); outBuf.destroy();
  return r;
}

function compare(got, want, what) {
  let num = 0, den = 0;
  for (let i = 0; i < want.length; i++) {
    const d = got[i] - want[i];
    num += d * d; den += want[i] * want[i];
    assert(Math.abs(d) <= 4e-3 + 4e-3 * Math.abs(want[i]), what + ": element " + i + " got " + got[i] + " want " + want[i]);
  }
  const l2 = Math.sqrt(num / den);
  console.log("       " + what + ": rel_l2=" + l2.toExponential(3));
  assert(l2 < 1e-5, what + ": rel_l2 " + l2);
}

test("plan creation: descriptor type 12, real sizes, rejections keep their messages", async () => {
  const r = fft.resolvePlanOptions({ type: "fftconv", shape: [1000], batch: 3, layout: REAL, fftConv: { boundary: "linear-full", kernelCount: 2, kernelShape: [31] } });
  assert(r.desc.type === 12 && r.meta.real === true, "type " + r.desc.type);
  assert(r.meta.outputShape[0] === 1030 && r.meta.inputBytes === 12000 && r.meta.kernelBytes === 248 && r.meta.outputBytes === 4 * 3 * 2 * 1030, JSON.stringify(r.meta));
  assert(fft.resolvePlanOptions({ type: "fftconv", shape: [8], layout: { interleavedComplex: true } }).desc.type === 3);
  assertThrows(() => fft.resolvePlanOptions({ type: "fftconv", shape: [8], layout: REAL, inPlace: true }), /^fftconv inPlace=true is not supported in current implementation$/);
  assertThrows(() => fft.resolvePlanOptions({ type: "fftconv", shape: [8], layout: REAL, precision: "f16-storage" }), /^fftconv supports precision:"f32" only in current implementation$/);
  assertThrows(() => fft.resolvePlanOptions({ type: "fftconv", shape: [8], layout: REAL, ioView: { input: { shape: [4], offset: [0] } } }), /^ioView is not an fftconv option/);
  assertThrows(() => fft.createFftConvChannelLanePreset({ shape: [8], batch: 2, kernelCount: 2, layout: REAL, input: { channels: 2 }, output: { channels: 2 } }),
    /interleavedComplex must be true for fftconv channel-lane presets/);
  const dev = await ensureDevice();
  const plan = fft.createPlan(dev, { type: "fftconv", shape: [256], batch: 2, layout: REAL, fftConv: { kernelCount: 2 } });
  assert(/lines-rconv\[N=256\]/.test(plan._route) && plan._launchesPerExec === 3, "route " + plan._route);
  const inBuf = dev.createBuffer({ size: 2 * 256 * 4, usage: usage() }), outBuf = dev.createBuffer({ size: 2 * 2 * 256 * 4, usage: usage() });
  const enc = dev.createCommandEncoder();
  assertThrows(() => plan.exec(enc, { input: inBuf, output: outBuf, kernel: new Float32Array(2 * 2 * 256) }), /^kernel Float32Array length must be 512 for kernelCount=2; got 1024$/);
  assertThrows(() => plan.exec(enc, { input: inBuf, output: outBuf, kernel: [new Float32Array(256)] }), /^kernel array length must equal fftConv.kernelCount=2; got 1$/);
  assertThrows(() => plan.exec(enc, { input: inBuf, output: outBuf, kernel: [new Float32Array(256), new Float32Array(512)] }), /^kernel\[1\] Float32Array length must be 256; got 512$/);
  plan.destroy(); inBuf.destroy(); outBuf.destroy();
});

test("lines-rconv: 1000 (*) 31 linear-same correlation, K = 2, batch-major, kernels as a list", async () => {
  const n = 1000, kn = 31, batch = 5, K = 2, off = (kn - 1) >> 1;
  const x = randomReal(n * batch, 11), h = [randomReal(kn, 12), randomReal(kn, 13)];
  const opts = { type: "fftconv", shape: [n], batch, layout: REAL, fftConv: { mode: "correlation", boundary: "linear-same", kernelCount: K, kernelShape: [kn], outputLayout: "batch-major" } };
  const r = await runPlan(opts, x, h, batch * K * n);
  assert(/pad\[1030->2048\] .*lines-rconv\[N=2048\]/.test(r.route) && r.launches === 1 + K, "route " + r.route + " launches " + r.launches);
  const want = new Float64Array(batch * K * n);
  for (let b = 0; b < batch; b++) for (let k = 0; k < K; k++) for (let m = 0; m < n; m++) {
    let acc = 0;
    const idx = m + off;                    // index into the logical FFT domain [0, n + kn - 1): lag idx below n, lag idx - (n + kn - 1) above
    const L = idx < n ? idx : idx - (n + kn - 1);
    for (let j = 0; j < kn; j++) { const p = j + L; if (p >= 0 && p < n) acc += x[b * n + p] * h[k][j]; }
    want[(b * K + k) * n + m] = acc;
  }
  compare(r.out, want, r.route.trim());
});

test("rconv[K]: rank 2, 24 x 10 (*) 5 x 3 linear-full convolution", async () => {
  const s0 = 24, s1 = 10, k0 = 5, k1 = 3, batch = 3, o0 = s0 + k0 - 1, o1 = s1 + k1 - 1;
  const x = randomReal(s0 * s1 * batch, 21), h = randomReal(k0 * k1, 22);
  const opts = { type: "fftconv", shape: [s0, s1], batch, layout: REAL, fftConv: { boundary: "linear-full", kernelCount: 1, kernelShape: [k0, k1] } };
  const r = await runPlan(opts, x, h, batch * o0 * o1);
  assert(/rconv\[K=1\]/.test(r.route) && !/lines-rconv/.test(r.route), "route " + r.route);
  const want = new Float64Array(batch * o0 * o1);
  for (let b = 0; b < batch; b++) for (let m1 = 0; m1 < o1; m1++) for (let m0 = 0; m0 < o0; m0++) {
    let acc = 0;
    for (let j1 = 0; j1 < k1; j1++) for (let j0 = 0; j0 < k0; j0++) {
      const p0 = m0 - j0, p1 = m1 - j1;
      if (p0 >= 0 && p0 < s0 && p1 >= 0 && p1 < s1) acc += x[(b * s1 + p1) * s0 + p0] * h[j1 * k0 + j0];
    }
    want[(b * o1 + m1) * o0 + m0] = acc;
  }
  compare(r.out, want, r.route.trim());
});

run();
