#!/usr/bin/env python3
"""Times the surface normals from a disparity map (adc_normals_device: the cleared report words, k_normals, the pinned read-back) on
one MI355X at 1920x1080, prices its traffic against the copy kernel and checks that the benchmark's headline did not move; writes
profiles/normals_timing.md.

    python tools/normals_timing.py [--parent-lib DIR/libadcensus_hip.so --parent-commit HASH] [--out profiles/normals_timing.md]

The driver starts one child process per step (this file with --child calls, or bench.py for the headline), each with its own time
limit, and stops at the first step that fails.
  calls     per map (the final maps a Match delivers for the benchmark's structured and noise pairs, D = 128), radius (1, 2, 3, 7;
            max_diff 1.0, min_points 5) and outputs (normals alone, normals8 alone, both): N calls enqueued back to back on the handle's
            stream, one adc_wait, best of --reps; the report is checked against the definition (tests/normals_ref.py).  The bytes the
            call moves stand next to the time -- 4 P in, 16 P and / or 4 P out -- and next to the time the copy kernel
            (adc_device_copy_kernel_ms) takes to move the same bytes (a copy of half of them: read + write)
  headline  bench.py --gpus 1 of the parent build and of this build (ADC_HIP_LIB selects the library), --reps repetitions each,
            alternating; the new median is judged against the min-max spread of the parent's own repetitions"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, D = 1920, 1080, 128
N = W * H
CALIB = (0.8 * W, 0.16, W / 2 - 0.3, H / 2 + 0.2, 1.25)
MAPS = ["structured", "noise"]
RADII = [1, 2, 3, 7]
OUTPUTS = [("normals", 16), ("normals8", 4), ("both", 20)]
TAG = "NORMALS_TIMING "


def child(a):
    import adcensus_amd as A
    from adcensus_amd import workloads
    from tests import normals_ref as R
    L = A.lib()
    out = {"version": L.adc_version().decode()}
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, A.ADCensusOption(max_disparity=D)), A.last_error()
    dm, dn, d8 = (L.adc_device_malloc(s) for s in (4 * N, 16 * N, 4 * N))
    ca, cb = L.adc_device_malloc(12 * N), L.adc_device_malloc(12 * N)
    for _, nbytes in OUTPUTS:  # the copy kernel on the bytes a call moves: a copy of n bytes reads n and writes n
        total = 4 * N + nbytes * N
        out["copy %d" % total] = float(L.adc_device_copy_kernel_ms(cb, ca, total // 2, 5))
    for name in MAPS:
        left, right = workloads.structured_pair(W, H, D, seed=777) if name == "structured" else workloads.noise_pair(W, H, 12345)
        disp = st.match(left, right)
        assert L.adc_memcpy_h2d(dm, disp.ctypes.data, disp.nbytes) == 0
        out[name + " usable"] = int(R.quantise(disp)[0].sum())
        for r in RADII:
            params = A.NormalsParams(r, 1.0, 5)
            want = R.normals(disp, CALIB, r, 1.0, 5)[2] if (r in (1, 2) or a.check_all) else None
            for oname, _ in OUTPUTS:
                pn, p8 = (dn if oname != "normals8" else None), (d8 if oname != "normals" else None)
                best = 1e9
                for _ in range(a.reps + 1):
                    t0 = time.perf_counter()
                    for _ in range(a.batch):
                        assert st.normals_device(dm, CALIB, params, pn, p8), A.last_error()
                    assert st.wait(), A.last_error()
                    best = min(best, (time.perf_counter() - t0) * 1e3 / a.batch)
                rep = st.normals_report()
                if want is not None:
                    assert [rep.usable, rep.fitted, rep.few_points, rep.degenerate] == R.report_words(want), (name, r, oname)
                out["%s r%d %s" % (name, r, oname)] = best
                out["%s r%d fitted" % (name, r)] = int(rep.fitted)
    for b in (dm, dn, d8, ca, cb):
        L.adc_device_free(b)
    st.Release()
    print(TAG + json.dumps(out), flush=True)


def run_child(cmd, lib, limit, tag):
    env = dict(os.environ, ADC_HIP_LIB=lib) if lib else dict(os.environ)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith(tag)]
    if r.returncode != 0 or not lines:
        print("step %s failed (exit %d): %s" % (" ".join(cmd[1:]), r.returncode, (r.stdout + r.stderr)[-2000:]), flush=True)
        sys.exit(1)  # (nothing more is started on the GPU behind a step that failed)
    print("step %s ok" % " ".join(cmd[1:]), flush=True)
    return json.loads(lines[-1][len(tag):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-all", action="store_true", help="calls: check the report of every radius against the definition (default: r = 1 and 2; the numpy definition takes a minute per map at r = 7)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_timing.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = os.path.abspath(__file__)
    md = ["# Surface normals from a disparity map: timing on one MI355X, 1920x1080", "",
          "`tools/normals_timing.py`; the final maps of the benchmark's structured and noise pairs (D = 128), max_diff 1.0, min_points 5; %d calls "
          "(`adc_normals_device`: the cleared report words, `k_normals`, the pinned read-back) enqueued back to back and one `adc_wait`, best of %d, ms per "
          "call.  P = 2073600 pixels; a call moves 4 P bytes in and 16 P (normals), 4 P (normals8) or 20 P (both) out.  Copy kernel: "
          "`adc_device_copy_kernel_ms` moving the same bytes (a copy of half of them, read + write)." % (a.batch, a.reps), ""]
    calls = run_child([sys.executable, me, "--child", "calls", "--batch", str(a.batch), "--reps", str(a.reps)] + (["--check-all"] if a.check_all else []), "", 900, TAG)
    md += ["| map | usable pixels | radius | fitted | outputs | MB moved | ms per call | GB/s | copy kernel, same bytes, ms | call / copy |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name in MAPS:
        for r in RADII:
            for oname, nbytes in OUTPUTS:
                total = 4 * N + nbytes * N
                t, c = calls["%s r%d %s" % (name, r, oname)], calls["copy %d" % total]
                md.append("| %s | %d | %d | %d | %s | %.1f | %.4f | %.0f | %.4f | %.2f |" % (name, calls[name + " usable"], r, calls["%s r%d fitted" % (name, r)], oname, total / 1e6, t,
                                                                                         total / t / 1e6, c, t / c if c > 0 else float("nan")))
    md += ["", "## The benchmark's headline against the parent (%s), %d alternating repetitions each" % (a.parent_commit, a.reps), ""]
    if a.parent_lib:
        new_lib = os.path.join(ROOT, "adcensus_amd", "lib", "libadcensus_hip.so")
        bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup), "--no-cpu-baseline"]
        runs = {"parent": [], "new": []}
        for _ in range(a.reps):
            for tag, lib in (("parent", a.parent_lib), ("new", new_lib)):
                runs[tag].append(bench_value(bench, lib))
        p, n = runs["parent"], runs["new"]
        med = statistics.median(n)
        verdict = "yes" if min(p) <= med <= max(p) else ("outside: " + ("above" if med > max(p) else "below"))
        md += ["`bench.py --gpus 1 --steps %d --warmup %d --no-cpu-baseline`, pairs/s at 1920x1080 D = 128; the library is selected with `ADC_HIP_LIB`; within a "
               "repetition the parent runs first." % (a.steps, a.warmup), "",
               "| parent repetitions | parent min - max | new repetitions | new median | inside the parent's spread |", "|---|---|---|---|---|",
               "| %s | %.2f - %.2f | %s | %.2f | %s |" % (" ".join("%.2f" % v for v in p), min(p), max(p), " ".join("%.2f" % v for v in n), med, verdict)]
    else:
        md.append("not measured (no parent library given)")
    text = "\n".join(md) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


def bench_value(cmd, lib):
    """one bench.py run with the given library -> its headline value (the last JSON line it prints)"""
    r = subprocess.run(["timeout", "-k", "10", "600"] + cmd, capture_output=True, text=True, env=dict(os.environ, ADC_HIP_LIB=lib), cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    if r.returncode != 0 or not lines:
        print("bench.py failed (exit %d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]), flush=True)
        sys.exit(1)  # (nothing more is started on the GPU behind a step that failed)
    v = float(json.loads(lines[-1])["value"])
    print("bench.py with %s: %.3f pairs/s" % (lib, v), flush=True)
    return v


if __name__ == "__main__":
    main()
