// GPU tier: fftConv.groups (grouped and depthwise convolution, y[b][k] = sum_{c < Cg} x[b][g Cg + c] (*) h[k][c], g = floor(k / Kg)) through the JavaScript host ->
// N-API addon -> C ABI.  Run by tests/test_js_fftconv_group.py.  The grouped tile kernel on 150 x 100 (*) 9 x 5 (C = 4, K = 4, G = 2, the 64-point tile forced) and
// the composed route on 1000 (*) 31 (C = 4, K = 2, G = 2), each against direct sums in float64 computed here; the kernel-list form of exec; the host's validation.
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

function withEnv(name, value, f) {
  const saved = process.env[name];
  if (value !== null) process.env[name] = value;
  try { return f(); } finally { if (value !== null) { if (saved === undefined) delete process.env[name]; else process.env[name] = saved; } }
}

// linear-same convolution, kernel-major: output o is index m = o + c of the logical domain, c = floor((M - 1) / 2).  Input line b * C + c is channel c of item b;
// kernel (k, c) is entry k * Cg + c and reads channel floor(k / Kg) * Cg + c
async function check(name, shape, ks, batch, C, K, G, sw, tag, launches, kernelList) {
  const [n0, n1] = [shape[0], shape[1] || 1], [m0, m1] = [ks[0], ks[1] || 1];
  const n = n0 * n1, kn = m0 * m1, Cg = C / G, Kg = K / G;
  const x = randomInterleaved(n * batch * C, 71), h = randomInterleaved(kn * K * Cg, 72);
  const opts = { type: "fftconv", shape, batch, fftConv: { mode: "convolution", boundary: "linear-same", kernelCount: K, kernelShape: ks, inputChannels: C, groups: G } };
  const dev = await ensureDevice();
  const inBuf = dev.createBuffer({ size: x.byteLength, usage: usage() });
  dev.queue.writeBuffer(inBuf, 0, x);
  const outFloats = 2 * K * batch * n;
  const outBuf = dev.createBuffer({ size: outFloats * 4, usage: usage() });
  const plan = withEnv("MI355FFT_GROUP_OLS2D", sw, () => fft.createPlan(dev, opts));
  assert(plan._route.includes(tag) && (launches === null || plan._launchesPerExec === launches), "route " + plan._route + " launches " + plan._launchesPerExec);
  assert(plan.groups === G && plan.inputChannels === C, "meta.groups " + plan.groups);
  const kernel = kernelList ? Array.from({ length: K * Cg }, (_, i) => h.subarray(2 * kn * i, 2 * kn * (i + 1))) : h;
  const enc = dev.createCommandEncoder();
  plan.exec(enc, { input: inBuf, output: outBuf, kernel });
  dev.queue.submit([enc.finish()]);
  await dev.queue.onSubmittedWorkDone();
  await outBuf.mapAsync(GPUMapMode.READ, 0, outFloats * 4);
  const got = new Float32Array(outBuf.getMappedRange(0, outFloats * 4).slice(0));
  outBuf.unmap();
  const c0 = (m0 - 1) >> 1, c1 = (m1 - 1) >> 1;
  let num = 0, den = 0;
  for (let k = 0; k < K; k++) for (let b = 0; b < batch; b++) for (let o1 = 0; o1 < n1; o1++) for (let o0 = 0; o0 < n0; o0++) {
    let re = 0, im = 0;
    const first = Math.floor(k / Kg) * Cg;
    for (let c = 0; c < Cg; c++) for (let r1 = 0; r1 < m1; r1++) {
      const p1 = o1 + c1 - r1;
      if (p1 < 0 || p1 >= n1) continue;
      for (let r0 = 0; r0 < m0; r0++) {
        const p0 = o0 + c0 - r0;
        if (p0 < 0 || p0 >= n0) continue;
        const xa = 2 * (((b * C + first + c) * n1 + p1) * n0 + p0), ha = 2 * (((k * Cg + c) * m1 + r1) * m0 + r0);
        re += x[xa] * h[ha] - x[xa + 1] * h[ha + 1]; im += x[xa] * h[ha + 1] + x[xa + 1] * h[ha];
      }
    }
    const at = 2 * (((k * batch + b) * n1 + o1) * n0 + o0), dr = got[at] - re, di = got[at + 1] - im;
    num += dr * dr + di * di; den += re * re + im * im;
    assert(Math.abs(dr) <= 4e-3 + 4e-3 * Math.abs(re) && Math.abs(di) <= 4e-3 + 4e-3 * Math.abs(im),
           name + " kernel " + k + " item " + b + " element " + o0 + "," + o1 + " got " + got[at] + "," + got[at + 1] + " want " + re + "," + im);
  }
  const l2 = Math.sqrt(num / den);
  console.log("       " + plan._route.trim() + ": rel_l2=" + l2.toExponential(3));
  assert(l2 <= 1e-5, "rel_l2 " + l2);
  // the length errors name the count as kernelCount=K x inputChannels/groups=Cg
  const enc2 = dev.createCommandEncoder();
  let msg = "";
  try { plan.exec(enc2, { input: inBuf, output: outBuf, kernel: h.subarray(0, 2 * kn * K) }); } catch (e) { msg = String(e.message); }
  assert(msg.includes("for kernelCount=" + K + " x inputChannels/groups=" + Cg), "packed length: " + msg);
  msg = "";
  try { plan.exec(enc2, { input: inBuf, output: outBuf, kernel: Array.from({ length: K }, (_, i) => h.subarray(2 * kn * i, 2 * kn * (i + 1))) }); } catch (e) { msg = String(e.message); }
  assert(msg.includes("kernel array length must equal fftConv.kernelCount=" + K + " x inputChannels/groups=" + Cg + "; got " + K), "list length: " + msg);
  plan.destroy(); inBuf.destroy(); outBuf.destroy();
}

test("tiles-conv-ols-group: 150 x 100 (*) 9 x 5 linear-same, batch 2, C = 4, K = 4, G = 2, the 64-point tile forced", async () => {
  await check("150x100", [150, 100], [9, 5], 2, 4, 4, 2, "64", "tiles-spectrum[N=64x64] tiles-conv-ols-group[N=64x64,L=56x60,C=4,G=2,K=4]", 2, false);
});

test("fftconv-sum with groups: 1000 (*) 31 linear-same, batch 2, C = 4, K = 2, G = 2, kernels as a list of K Cg arrays", async () => {
  await check("1000", [1000], [31], 2, 4, 2, 2, null, "fftconv-sum[K=2,C=4,G=2]", null, true);
});

test("fftConv.groups: validation", async () => {
  const dev = await ensureDevice();
  const base = (fc) => ({ type: "fftconv", shape: [64, 48], batch: 2,
    fftConv: Object.assign({ boundary: "linear-same", kernelCount: 4, kernelShape: [5, 5], inputChannels: 4 }, fc) });
  const fails = (opts, text) => { let msg = ""; try { fft.createPlan(dev, opts).destroy(); } catch (e) { msg = String(e.message); } assert(msg.includes(text), text + ": " + msg); };
  for (const bad of [0, -1, 1.5, "2", true]) fails(base({ groups: bad }), "fftConv.groups must be a positive integer");
  fails(base({ groups: 3 }), "fftConv.groups=3 must divide fftConv.inputChannels=4");
  fails(base({ groups: 2, kernelCount: 3 }), "fftConv.groups=2 must divide fftConv.kernelCount=3");
  fails(base({ groups: 2, channelPolicy: { input: { preset: "nchw" } } }), "fftConv.inputChannels > 1 cannot be combined with fftConv.channelPolicy.input");
  const one = fft.createPlan(dev, base({ groups: 1 })), none = fft.createPlan(dev, base({}));
  assert(one._route === none._route && one._launchesPerExec === none._launchesPerExec, one._route + " / " + none._route);
  one.destroy(); none.destroy();
});

run();
