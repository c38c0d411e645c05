"""bench.py's kernel workloads: the coefficient kernel (c2, c2_444, c2_unaligned, c3, c1) and the PNG row filters (c5), and their short-protocol measurements."""
from .common import *  # noqa: F401,F403
from .roofline import *  # noqa: F401,F403
from . import roofline as _roofline  # noqa: F401


QUICK_SETTLE_MS = 60.0  # the extras run behind host-bound phases (allocations, uploads, the oracle check): the clocks have dropped


# ------------------------------------------------------------------------------------------------------------------
# the coefficient kernel (c2, c2_444, c2_unaligned, c3, c1)
# ------------------------------------------------------------------------------------------------------------------
class CoeffWorkload:
    def __init__(self, job, name, quality):
        import numpy as np
        import synth
        from pixo_amd import jpeg
        self.job, self.name, self.q, self.jpeg, self.np = job, name, quality, jpeg, np
        torch = job.torch
        self.w, self.h, self.batch, self.ss, self.label = WORKLOADS[name]
        w, h, batch, ss = self.w, self.h, self.batch, self.ss
        self.yb, self.cbn = jpeg.coefficient_geometry(w, h, 2, ss)
        self.in_bytes = w * h * 3 * batch
        self.out_bytes = (self.yb + 2 * self.cbn) * 128 * batch
        # rotate over enough buffer sets that the working set exceeds the 256 MiB Infinity Cache
        self.nbuf = min(64, max(2, -(-(640 << 20) // (self.in_bytes + self.out_bytes))))
        self.base = synth.noise(w, h, 42 + job.rank)
        if job.stub:
            self.ins = self.outs = None
            return
        host = torch.from_numpy(np.ascontiguousarray(self.base))
        dev = job.dev
        self.ins, self.outs = [], []
        for i in range(self.nbuf):
            t = host.to(dev)
            if batch > 1:
                t = t.repeat(batch)
            t = t ^ torch.tensor(i & 0xFF, dtype=torch.uint8, device=dev) if i else t  # distinct content per buffer
            self.ins.append(t.contiguous())
            self.outs.append((torch.empty((batch * self.yb, 64), dtype=torch.int16, device=dev),
                              torch.empty((batch * self.cbn, 64), dtype=torch.int16, device=dev),
                              torch.empty((batch * self.cbn, 64), dtype=torch.int16, device=dev)))
        self.stream = torch.cuda.current_stream().cuda_stream

    def step(self, i):
        if self.job.stub:
            time.sleep(2e-5)
            return
        k = i % self.nbuf
        y, cb, cr = self.outs[k]
        self.jpeg.coefficients_device(self.ins[k], self.w, self.h, 2, self.ss, self.q, y, cb, cr, batch=self.batch, stream=self.stream)

    def outputs(self, i):
        """what step(i) handed its caller: the quantised Y, Cb and Cr blocks (int16, 64 per row, images of a batch one after
        the other)"""
        self.job.sync()
        y, cb, cr = self.outs[i % self.nbuf]
        return [("y", y.cpu().numpy()), ("cb", cb.cpu().numpy()), ("cr", cr.cpu().numpy())]

    def check(self):
        """correctness inside the bench: buffer 0 against the oracle on a 64-row strip (Y, Cb and Cr)"""
        import oracle_lib as O
        np = self.np
        strip_h = 64
        oy, ocb, ocr = O.coeffs(self.base[: self.w * strip_h * 3], self.w, strip_h, 2, self.ss, self.q)
        self.step(0)
        self.job.sync()
        gy = self.outs[0][0][: oy.shape[0]].cpu().numpy()
        gcb = self.outs[0][1][: ocb.shape[0]].cpu().numpy()
        gcr = self.outs[0][2][: ocr.shape[0]].cpu().numpy()
        if not (np.array_equal(gy, oy) and np.array_equal(gcb, ocb) and np.array_equal(gcr, ocr)):
            raise SystemExit("bench: GPU coefficients differ from the oracle — refusing to report a number")

    def roofline(self, kernel_ms, copy_ms=None):
        alg = self.in_bytes + self.out_bytes  # 3 B/px read + 3 B/px written (4:2:0); 3 + 6 for 4:4:4
        achieved = alg / (kernel_ms * 1e-3) / 1e9
        traffic, src = traffic_of(self.name)
        issue = issue_of(self.name, kernel_ms * 1e3)
        # `bound` is COMPUTED: the larger of the two fractions of this run (HBM bytes against 8 TB/s, vector instructions
        # against what 1,024 SIMDs issue) names the roofline that binds
        r = {"bound": bound_of(achieved / HBM_PEAK_GBPS, issue), "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
             "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic, "traffic_source": src, **issue,
             "kernel": "jpeg_coeffs_kernel<%s, %s>" % ("M420" if self.ss else "M444", "L_FUNNEL" if self.w * 3 % 4 else "L_ALIGNED"),
             "algorithmic_bytes_per_launch": alg, "kernel_us_avg": round(kernel_ms * 1e3, 3),
             "read_only_frac_of_peak": round(self.in_bytes / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)}
        if copy_ms:
            # the plain copy of the same bytes in the same launch shape, timed in THIS run by the same block protocol
            # (pixo_hip_debug_stream_copy): what the memory system of this box, at this moment, gives 50 MB in + 50 MB out
            r["copy_us_same_run"] = round(copy_ms * 1e3, 3)
            r["copy_GBps_same_run"] = round(alg / (copy_ms * 1e-3) / 1e9, 1)
            r["copy_frac_of_peak_same_run"] = round(alg / (copy_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
            r["kernel_over_copy_same_run"] = round(kernel_ms / copy_ms, 4)
            r["frac_of_copy_same_run"] = round(copy_ms / kernel_ms, 4)
            # with the memory system's own ceiling measured in the same run, `bound` compares like with like: the kernel's share of
            # what a plain copy of its bytes gets against its share of the issue rate (a kernel at 0.99 of the copy and 0.82 of the
            # issue rate is bound by the memory system, although 0.71 of the 8 TB/s PEAK is the smaller number)
            r["bound"] = bound_of(copy_ms / kernel_ms, issue)
            r["bound_rule"] = "larger of frac_of_copy_same_run and frac_issue"
        return r

    def copy_step_factory(self):
        """A plain copy of this workload's bytes (4:2:0: as many out as in) over the same rotating input buffers."""
        if self.in_bytes != self.out_bytes or self.in_bytes % 24576:
            return None
        torch = self.job.torch
        outs = [torch.empty(self.in_bytes, dtype=torch.uint8, device=self.job.dev) for _ in range(self.nbuf)]
        jpeg, ins, n, nb, stream = self.jpeg, self.ins, self.in_bytes, self.nbuf, self.stream

        def step(i):
            k = i % nb
            jpeg.debug_stream_copy(ins[k], outs[k], n, stream=stream)
        step.outs = outs
        return step


# ------------------------------------------------------------------------------------------------------------------
# c5: PNG row filters
# ------------------------------------------------------------------------------------------------------------------
class PngWorkload:
    def __init__(self, job):
        import synth
        from pixo_amd import png
        torch = job.torch
        self.job, self.png = job, png
        self.w = self.h = 4096
        self.bpp = 4
        self.base = synth.rgba_noise_alpha1(self.w, self.h, 42 + job.rank)
        self.in_bytes, self.out_bytes = self.w * self.h * self.bpp, png.filtered_size(self.w, self.h, self.bpp)
        self.nbuf = 5  # 5 x 134 MB > Infinity Cache
        host = torch.from_numpy(self.base)
        dev = job.dev
        self.ins = [(host.to(dev) ^ torch.tensor(i, dtype=torch.uint8, device=dev)).contiguous() for i in range(self.nbuf)]
        self.outs = [torch.empty(self.out_bytes, dtype=torch.uint8, device=dev) for _ in range(self.nbuf)]
        self.sums = [torch.zeros(2 * self.h, dtype=torch.int64, device=dev) for _ in range(self.nbuf)]
        self.scratch = torch.zeros(4, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream

    def step(self, i):
        k = i % self.nbuf
        self.png.apply_filters_async(self.ins[k], self.w, self.h, self.bpp, self.outs[k], self.sums[k], self.scratch,
                                     self.png.FilterStrategy.ADAPTIVE, 0, self.stream)

    def outputs(self, i):
        """what step(i) handed its caller: the filtered stream (a filter byte + the filtered row, row by row), the per-row
        Adler-32 sums and the Adler-32 they make"""
        import numpy as np
        self.job.sync()
        k = i % self.nbuf
        sums = self.sums[k].cpu().numpy()
        adler = self.png.adler32_from_row_sums(sums.view(np.uint64), self.w, self.h, self.bpp)
        filtered = self.outs[k].cpu().numpy().reshape(self.h, -1)
        return [("filtered", filtered), ("row_sums", sums.reshape(self.h, 2)), ("adler32", np.array([adler], dtype=np.int64))]

    def check(self):
        """buffer 0 against the reference-made vector of SURVEY §8c (rank 0's input is that very image)"""
        import numpy as np
        self.step(0)
        self.job.sync()
        adler = self.png.adler32_from_row_sums(self.sums[0].cpu().numpy().view(np.uint64), self.w, self.h, self.bpp)
        digest = hashlib.sha256(self.outs[0].cpu().numpy().tobytes()).hexdigest()
        if self.job.rank == 0 and (adler != 0x90CC12E3 or not digest.startswith("240e005d4da54561")):
            raise SystemExit("bench: filtered stream differs from the reference's — refusing to report a number")


def quick_kernel(job, name, q, steps=200, blocks=7):
    """One of the other configurations, measured the way the metric is: the workload's own launches keep the GPU busy for
    QUICK_SETTLE_MS first (each of these follows a host-bound phase — building the buffers, the oracle check — during which
    the clocks fall), then warmup, then the median of `blocks` blocks of `steps` steps; kernel time from HIP events."""
    wl = CoeffWorkload(job, name, q)
    wl.check()
    job.settle(wl.step, QUICK_SETTLE_MS)
    _, evs = job.time_blocks(wl.step, steps, 20, blocks)
    kernel_ms = statistics.median(evs) / steps
    r = wl.roofline(kernel_ms)
    out = {"workload": wl.label, "kernel_us": r["kernel_us_avg"], "Mpixels_per_s": round(wl.w * wl.h * wl.batch / kernel_ms / 1e3, 1),
           "achieved_GBps": r["achieved"], "frac": r["frac"], "bound": r["bound"], "steps": steps, "blocks": blocks, "settle_ms": QUICK_SETTLE_MS}
    for key in ("frac_issue", "valu_insts_per_launch", "issue_source", "counters_stale", "counters_stale_reason", "engine_clock_GHz", "valu_busy_under_counters",
                "traffic", "traffic_source"):
        if key in r:
            out[key] = r[key]
    in_bytes, out_bytes = wl.in_bytes, wl.out_bytes
    del wl
    job.torch.cuda.empty_cache()
    # the plain copy of the same bytes (50 -> 100 MB for 4:4:4, 398 -> 401 MB for the batch ...) right behind the kernel's blocks
    with_copy(job, out, in_bytes, out_bytes, out["kernel_us"], r, steps=max(20, min(steps, int(2e5 / max(out["kernel_us"], 1.0)))))
    return out


def quick_png(job, steps=100, blocks=7):
    wl = PngWorkload(job)
    wl.check()
    job.settle(wl.step, QUICK_SETTLE_MS)
    _, evs = job.time_blocks(wl.step, steps, 20, blocks)
    kernel_ms = statistics.median(evs) / steps
    alg = wl.in_bytes + wl.out_bytes
    issue = issue_of("c5", kernel_ms * 1e3)
    frac = alg / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS
    out = {"workload": "configs[4]: 4096x4096 RGBA8 PNG row filters (Adaptive) + Adler-32 partials", "kernel_us": round(kernel_ms * 1e3, 3),
           "Mpixels_per_s": round(4096 * 4096 / kernel_ms / 1e3, 1), "achieved_GBps": round(alg / (kernel_ms * 1e-3) / 1e9, 1),
           "frac": round(frac, 4), "bound": bound_of(frac, issue), **issue, "steps": steps, "blocks": blocks}
    traffic, src = traffic_of("c5")
    out["traffic"], out["traffic_source"] = traffic, src
    in_bytes, out_bytes = wl.in_bytes, wl.out_bytes
    del wl
    job.torch.cuda.empty_cache()
    with_copy(job, out, in_bytes, out_bytes, out["kernel_us"], issue, steps=steps)
    return out


__all__ = [n for n in dir() if not n.startswith("__")]
