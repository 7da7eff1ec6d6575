// GPU tier: precision "f16-storage" through the JavaScript host -> N-API addon -> C ABI.  Binary16 data travels as raw bytes
// (Uint16Array).  Run by tests/test_js_f16_storage.py, which hands in the input bytes of each case (argv[2] = a directory
// with <case>.in.bin) and compares the <case>.out.bin files written here with the Python host's output for the same plan.
// The ioView case follows the reference's complete.suite.js:4395-4460 (sentinel output, clearOutside: false).
import fs from "fs";
import path from "path";
import { test, assert, assertThrows, run } from "./harness.mjs";
import * as fft from "../index.js";

const dir = process.argv[2];
let device = null;
async function ensureDevice() { if (!device) device = await fft.requestDevice(); return device; }
const readU16 = (name) => { const b = fs.readFileSync(path.join(dir, name)); return new Uint16Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const usage = () => GPUBufferUsage.STORAGE | GPUBufferUsage.COPY_SRC | GPUBufferUsage.COPY_DST;

async function runCase(name, opts, outBytes, outInit) {
  const dev = await ensureDevice();
  const input = readU16(name + ".in.bin");
  const inBuf = dev.createBuffer({ size: input.byteLength, usage: usage() });
  dev.queue.writeBuffer(inBuf, 0, input);
  const outBuf = dev.createBuffer({ size: outBytes, usage: usage() });
  if (outInit) dev.queue.writeBuffer(outBuf, 0, outInit);
  const plan = fft.createPlan(dev, Object.assign({ layout: { interleavedComplex: true }, precision: "f16-storage" }, opts));
  const enc = dev.createCommandEncoder();
  plan.exec(enc, { input: inBuf, output: outBuf });
  dev.queue.submit([enc.finish()]);
  await dev.queue.onSubmittedWorkDone();
  await outBuf.mapAsync(GPUMapMode.READ, 0, outBytes);
  const out = new Uint8Array(outBuf.getMappedRange(0, outBytes));
  outBuf.unmap();
  fs.writeFileSync(path.join(dir, name + ".out.bin"), out);
  const route = plan._route;
  plan.destroy(); inBuf.destroy(); outBuf.destroy();
  return { out: new Uint16Array(out.buffer, out.byteOffset, out.byteLength / 2), route };
}

test("device reports shader-f16", async () => {
  const dev = await ensureDevice();
  assert(dev.features.has("shader-f16"), "features: " + [...dev.features]);
});

test("f16-storage rejections carry the reference's messages", async () => {
  const dev = await ensureDevice();
  assertThrows(() => fft.createPlan(dev, { type: "c2c", shape: [8], direction: "forward", precision: "f16-storage", layout: { interleavedComplex: true, strides: [2] } }),
    /^custom strides currently support precision:"f32" only$/);
  assertThrows(() => fft.createPlan(dev, { type: "r2c", shape: [8], direction: "forward", precision: "f16-storage", layout: { interleavedComplex: true, strides: [2] } }),
    /^custom strides currently support precision:"f32" only for r2c$/);
  assertThrows(() => fft.createPlan(dev, { type: "fftconv", shape: [8], precision: "f16-storage" }),
    /^fftconv supports precision:"f32" only in current implementation$/);
});

test("c2c N=1024 f16-storage on the fused line launch", async () => {
  const r = await runCase("fused", { type: "c2c", shape: [1024], batch: 8, direction: "forward", normalize: "none" }, 1024 * 8 * 4);
  assert(r.route.trim().endsWith("f16"), "route " + r.route);
});

test("c2c f16-storage with ioView input+output, clearOutside=false keeps the sentinel", async () => {
  const viewOut = 32;
  const sentinel = new Uint16Array(2 * viewOut);
  for (let i = 0; i < viewOut; i++) { sentinel[2 * i] = 0x3e00; sentinel[2 * i + 1] = 0xc000; }    // 1.5, -2.0
  const r = await runCase("ioview", {
    type: "c2c", shape: [16], direction: "forward", batch: 1, inPlace: false, normalize: "none",
    ioView: { input: { shape: [8], placement: "center" }, output: { shape: [viewOut], placement: "center", clearOutside: false } },
  }, viewOut * 4, sentinel);
  assert(r.route.startsWith("f16-in"), "route " + r.route);
  for (let i = 0; i < viewOut; i++) {
    if (i >= 8 && i < 24) continue;
    assert(r.out[2 * i] === 0x3e00 && r.out[2 * i + 1] === 0xc000, "untouched view element " + i + " changed");
  }
});

run();
