// TEST INFRASTRUCTURE — not product code.
//
// Loader for the reference's own compiled artefact (oracle/_ref/pixo_bg.wasm, staged by `make -C oracle ref`), calling
// its export `resizeImage` (reference src/wasm.rs:183-201).  The wasm-bindgen ABI of that export is
//   resizeImage(retptr, ptr, len, src_width, src_height, dst_width, dst_height, color_type, algorithm)
// with the result (ptr, len, error object, is-error) stored at retptr.
//
// Usage (one process, many cases):
//   node tests/ref_resize_wasm.js <manifest.json>
// manifest = {"wasm": "...optional path...", "cases": [
//   {"input":"in.bin","sw":16,"sh":16,"dw":8,"dh":8,"color_type":2,"algorithm":2,"output":"out.bin","repeat":1}, ...]}
// Prints one JSON line per case: {"ok":true,"len":N,"ms":[...]} or {"ok":false,"error":"<message>"}.
'use strict';
const fs = require('fs');
const path = require('path');

function load(wasmPath) {
  const st = { lastErr: null, wasm: null };
  const imports = { wbg: {
    // the module's only import: builds a JsError from (ptr, len)
    __wbg_Error_52673b7de5a0ca89: (p, l) => {
      st.lastErr = Buffer.from(st.wasm.memory.buffer, p, l).toString();
      return 132;
    },
  } };
  st.wasm = new WebAssembly.Instance(new WebAssembly.Module(fs.readFileSync(wasmPath)), imports).exports;
  return st;
}

function resizeImage(st, data, c) {
  const wasm = st.wasm;
  const ret = wasm.__wbindgen_add_to_stack_pointer(-16);
  const ptr = wasm.__wbindgen_export(data.length, 1) >>> 0; // malloc(len, align); the callee takes ownership
  new Uint8Array(wasm.memory.buffer).set(data, ptr);
  st.lastErr = null;
  wasm.resizeImage(ret, ptr, data.length, c.sw, c.sh, c.dw, c.dh, c.color_type, c.algorithm);
  const dv = new DataView(wasm.memory.buffer);
  const out = dv.getInt32(ret, true) >>> 0;
  const len = dv.getInt32(ret + 4, true) >>> 0;
  const isErr = dv.getInt32(ret + 12, true);
  wasm.__wbindgen_add_to_stack_pointer(16);
  if (isErr) throw new Error(st.lastErr === null ? 'unknown error' : st.lastErr);
  const res = Buffer.from(new Uint8Array(wasm.memory.buffer).slice(out, out + len));
  wasm.__wbindgen_export2(out, len, 1); // free(ptr, len, align)
  return res;
}

function main() {
  const manifest = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
  const wasmPath = manifest.wasm || path.join(__dirname, '..', 'oracle', '_ref', 'pixo_bg.wasm');
  const st = load(wasmPath);
  for (const c of manifest.cases) {
    try {
      const data = new Uint8Array(fs.readFileSync(c.input));
      const ms = [];
      let out = null;
      for (let i = 0; i < (c.repeat || 1); i++) {
        const t0 = process.hrtime.bigint();
        out = resizeImage(st, data, c);
        ms.push(Number(process.hrtime.bigint() - t0) / 1e6);
      }
      if (c.output) fs.writeFileSync(c.output, out);
      console.log(JSON.stringify({ ok: true, len: out.length, ms }));
    } catch (e) {
      console.log(JSON.stringify({ ok: false, error: String(e.message) }));
    }
  }
}

main();
