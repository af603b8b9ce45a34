"""Wave timeline of the config-2 launch (65 536 pairs of 150 x 150: 2 048 waves at 38 columns per lane, one residency): when
every wave starts, enters its loop, leaves it, stores and retires, and which SIMD it shared with which other wave.  The batch
is the library's own (plan, image, records); the kernel is the stamped diagnostic build of tools/sw_wave_timeline.hip, launched
at workgroup sizes of 64, 256 and 512 threads on an idle device, scores checked against the library's every time.
    python tools/sw_wave_timeline.py [--out FILE] [--reps 3] [--build-only]
Per configuration one table, a row per XCD and one over all SIMDs.  Times in microseconds: a wave's cycle counter is the shader
clock; its rate is taken per XCD, and every CU's origin (the CUs' counters stand far apart), from the 100 MHz constant clock read
beside the first and last stamp.  Read the shares, not the lengths: the stamped build carries five counter reads with their waits
and fences.  Behind the tables: the unstamped body timed with HIP events at the three workgroup sizes, with the staged wave
priority (SwParams::stage) off and on."""
import argparse, ctypes as C, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sw_wave_timeline.hip")
LIB = os.path.join(HERE, "build", "libsw_wave_timeline.so")
CSRC = os.path.join(ROOT, "accelerating-genomics_amd", "csrc")


def build():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("agx_sw_pk2_kernel.inc", "agx_sw.h", "agx_sw_batch.h", "agx_internal.h")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps):
        return
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC",
                    "-I" + os.path.join(ROOT, "include"), SRC, "-o", LIB], check=True)


STAGES = {0: "no staging", 1: "s_setprio 3, 2, 1, 0 at 1/2, 3/4, 7/8 of the quads", 2: "s_setprio 3, 2, 1, 0 at equal quarters"}


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return (float(np.median(v)), float(v.max())) if v.size else (float("nan"), float("nan"))


def analyse(S):
    """S: n_waves x 8 stamp words -> rows (label, dict) per XCD and over all."""
    t = S[:, :5].astype(np.float64)
    r0, r1 = S[:, 5].astype(np.float64), S[:, 6].astype(np.float64)
    hw = S[:, 7] & 0xffffffff
    xcc = ((S[:, 7] >> 32) & 0xf).astype(np.int64)
    simd = (xcc << 16) | (hw & 0xff30).astype(np.int64)  # XCC, SE, SH, CU, SIMD
    cu = (xcc << 16) | (hw & 0xff00).astype(np.int64)
    us = np.zeros_like(t)  # every stamp on one time axis
    mhz = {}
    for x in np.unique(xcc):
        m = xcc == x
        mhz[int(x)] = float(np.median((t[m, 4] - t[m, 0]) / ((r1[m] - r0[m]) * 0.01)))  # cycles per microsecond
    # the cycle counters of different CUs stand far apart: every CU's waves are placed by the constant clock beside their entry
    # stamps (10 ns a tick: what is compared ACROSS CUs carries that much uncertainty, what is compared within one does not)
    for c in np.unique(cu):
        m = cu == c
        f = mhz[int(c >> 16)]
        rel = (t[m] - t[m, 0].min()) / f
        us[m] = rel + np.median(r0[m] * 0.01 - rel[:, 0])
    us -= us[:, 0].min()
    # the pairs of waves that shared a SIMD: older = the one that started first
    order = np.lexsort((us[:, 0], simd))
    s_sorted = simd[order]
    first = np.flatnonzero(np.r_[True, s_sorted[1:] != s_sorted[:-1]])
    count = np.diff(np.r_[first, s_sorted.size])
    old, young = order[first[count == 2]], order[first[count == 2] + 1]
    rows = []
    for label, wm in [("XCD %d" % x, xcc == x) for x in np.unique(xcc)] + [("all", np.ones(xcc.size, bool))]:
        pm = wm[old]
        o, y = old[pm], young[pm]
        loop = us[:, 2] - us[:, 1]
        d = dict(waves=int(wm.sum()), simds=int(np.unique(simd[wm]).size), paired=int(pm.sum()),
                 mhz=mhz[int(label[4:])] if label != "all" else float(np.median(list(mhz.values()))),
                 start_first=float(us[wm, 0].min()), start_last=float(us[wm, 0].max()),
                 start_gap=stats(us[y, 0] - us[o, 0]), head=stats(us[o, 1] - us[o, 0]), head_young=stats(us[y, 1] - us[y, 0]),
                 loop_old=stats(loop[o]), loop_young=stats(loop[y]), loop_all=stats(loop[wm]),
                 leave_gap=stats(us[y, 2] - us[o, 2]), retire_gap=stats(us[y, 4] - us[o, 4]),
                 epilogue=stats(us[wm, 3] - us[wm, 2]), store=stats(us[wm, 4] - us[wm, 3]), tail=stats(us[wm, 4] - us[wm, 2]),
                 leave_first=float(us[wm, 2].min()), leave_last=float(us[wm, 2].max()),
                 retire_first=float(us[wm, 4].min()), retire_last=float(us[wm, 4].max()))
        rows.append((label, d))
    return rows


def table(title, rows):
    mm = lambda p: "%.2f / %.2f" % p
    out = ["### " + title, "",
           "| | waves | SIMDs (pairs) | clock MHz | start first .. last | start gap in a SIMD (med / max) | head, older wave (med / max) | head, younger wave (med / max) | loop, older wave (med / max) "
           "| loop, younger wave (med / max) | younger leaves the loop later by (med / max) | younger retires later by (med / max) "
           "| last step -> store (med / max) | store -> taken (med / max) | tail = last step -> retire (med / max) | loop left first .. last | retire first .. last |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for label, d in rows:
        out.append("| %s | %d | %d (%d) | %.0f | %.2f .. %.2f | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %.2f .. %.2f | %.2f .. %.2f |" % (
            label, d["waves"], d["simds"], d["paired"], d["mhz"], d["start_first"], d["start_last"], mm(d["start_gap"]), mm(d["head"]), mm(d["head_young"]),
            mm(d["loop_old"]), mm(d["loop_young"]), mm(d["leave_gap"]), mm(d["retire_gap"]), mm(d["epilogue"]), mm(d["store"]), mm(d["tail"]),
            d["leave_first"], d["leave_last"], d["retire_first"], d["retire_last"]))
    a = rows[-1][1]
    out += ["", "younger wave leaves its loop later than the older by %.2f us median = %.2f %% of the loop (%.2f us)" % (
        a["leave_gap"][0], 100 * a["leave_gap"][0] / a["loop_all"][0], a["loop_all"][0]), ""]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    build()
    if args.build_only:
        return
    import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
    tl = C.CDLL(LIB)
    tl.sw_wave_timeline_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32]
    ctx = agx.Context(0)
    b = synth.sw_pairs(65536, 150, 150, seed=2, related_frac=0.25)
    dev = ctx.sw_batch(b)
    info = dev.info()
    dev.launch()
    want = dev.scores().copy()
    pinned = agx.host_array(b.n_pairs, np.int32)
    lines = ["# Wave timeline of the config-2 launch (tools/sw_wave_timeline.py)", "",
             "%d pairs of 150 x 150, %d waves, %s; times in us from the first wave's start; %d stamped launches per configuration, the last one shown"
             % (b.n_pairs, info.n_waves, agx.lib().agx_version().decode(), args.reps), ""]
    S = np.zeros((info.n_waves, 8), dtype=np.uint64)
    for wg, wide, bound, stage in ((256, 1, 0, 0), (64, 1, 0, 0), (512, 1, 0, 0), (256, 1, 1, 0), (256, 0, 0, 0), (256, 1, 0, 1), (256, 1, 1, 1), (256, 1, 0, 2)):
        spans = []
        for _ in range(args.reps):
            pinned[:] = -1
            rc = tl.sw_wave_timeline_run(dev._h, wg, wide, stage, pinned.ctypes.data if bound else None, S.ctypes.data, info.n_waves)
            if rc:
                raise SystemExit("sw_wave_timeline_run(wg %d, wide %d, bound %d, stage %d) -> %d" % (wg, wide, bound, stage, rc))
            got = pinned if bound else dev.scores()
            if not np.array_equal(got, want):
                raise SystemExit("wg %d wide %d bound %d: scores differ from the library's" % (wg, wide, bound))
            rows = analyse(S)
            spans.append(rows[-1][1]["retire_last"])
        title = "workgroup of %d threads, %s, %s, scores %s -- first start to last retire over the launches: %s us" % (
            wg, "period C / 2 (sw_fill_pk2w<38>'s body)" if wide else "period of four (sw_fill_pk2<38, 4>'s body)", STAGES[stage],
            "bound to page-locked host memory" if bound else "left in HBM", ", ".join("%.2f" % s for s in spans))
        lines += table(title, rows)
        print("\n".join(table(title, rows)), flush=True)
    # the experiments: the unstamped body at the three workgroup sizes, without and with the staged priority, kernel only
    tl.sw_wave_timeline_time.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]
    configs = [(256, 0), (64, 0), (512, 0), (256, 1), (256, 2), (64, 1), (512, 1)]
    names = STAGES
    res = {(c, bd): [] for c in configs for bd in (0, 1)}
    for rnd in range(3):  # alternating
        for bd in (0, 1):
            for wg, mode in configs:
                ms = C.c_float()
                pinned[:] = -1
                rc = tl.sw_wave_timeline_time(dev._h, wg, mode, 100, pinned.ctypes.data if bd else None, C.byref(ms))
                if rc:
                    raise SystemExit("sw_wave_timeline_time(wg %d, mode %d, bound %d) -> %d" % (wg, mode, bd, rc))
                if not np.array_equal(pinned if bd else dev.scores(), want):
                    raise SystemExit("wg %d mode %d bound %d: scores differ from the library's" % (wg, mode, bd))
                res[((wg, mode), bd)].append(ms.value * 1e3)
    ctx.sync()
    lib_us = []
    for rnd in range(3):
        ctx.timer_start()
        for _ in range(100):
            dev.launch()
        lib_us.append(ctx.timer_stop() * 10)
    ex = ["### The unstamped body, kernel only: 100 launches back to back, three alternating rounds (us per launch)", "",
          "| workgroup | priority | scores left in HBM | scores bound to page-locked host memory |", "|---|---|---|---|"]
    for wg, mode in configs:
        ex.append("| %d | %s | %s | %s |" % (wg, names[mode], " / ".join("%.2f" % v for v in res[((wg, mode), 0)]),
                                           " / ".join("%.2f" % v for v in res[((wg, mode), 1)])))
    ex.append("| 256 | the library's own launch (`sw_fill_pk2w<38>`, staging as the host chose it) | %s | |" % " / ".join("%.2f" % v for v in lib_us))
    ex.append("")
    lines += ex
    print("\n".join(ex), flush=True)
    dev.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
