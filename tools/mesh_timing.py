#!/usr/bin/env python3
"""Times the triangle mesh from a disparity map (adc_mesh_device: the cleared report words, k_mesh_measure, k_mesh_scan, k_mesh_emit,
the pinned read-back) on one MI355X at 1920x1080, prices its traffic against the copy kernel and checks that the benchmark's headline
did not move; writes profiles/mesh_timing.md.

    python tools/mesh_timing.py [--parent-lib DIR/libadcensus_hip.so --parent-commit HASH] [--out profiles/mesh_timing.md]

The driver starts one child process per step (this file with --child calls, or bench.py for the headline), each with its own time
limit, and stops at the first step that fails.
  calls     per map (the final maps a Match delivers for the benchmark's structured and noise pairs, D = 128, at max_diff 1.0; the
            noise map once more without a gate, the worst case), step (1, 2, 4) and outputs (everything: vertices with colours,
            vertex_index, triangles, the count words; vertices alone; triangles alone): one call between two HIP events on the
            handle's stream, best of --reps after a warm-up; the report is checked against the definition (tests/mesh_ref.py).  The
            bytes the call moves stand next to the time, and next to the time the copy kernel (adc_device_copy_kernel_ms) takes to
            move the same bytes (a copy of half of them: read + write)
  headline  bench.py --gpus 1 of the parent build and of this build (ADC_HIP_LIB selects the library), --reps repetitions each,
            alternating; the new median is judged against the min-max spread of the parent's own repetitions"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, D = 1920, 1080, 128
N = W * H
CALIB = (0.8 * W, 0.16, W / 2 - 0.3, H / 2 + 0.2, 1.25)
MAPS = [("structured", "structured", 1.0), ("noise", "noise", 1.0), ("noise, no gate", "noise", float("inf"))]
STEPS = [1, 2, 4]
OUTPUTS = ["everything", "vertices", "triangles"]
TAG = "MESH_TIMING "


def priced_bytes(lattice, vertices, triangles, outputs):
    """what a call really moves: the map read once per lattice point by the measure and once per vertex by the emit, the records
    written, the colours read, and the scratch (one code byte per lattice point written and read when triangles are asked for; per
    chunk of 64 lattice points the used word and the two counts, written, scanned and read back: 40 bytes)"""
    chunks = (lattice + 63) // 64
    total = 4 * lattice + 40 * chunks
    if outputs in ("everything", "vertices"):
        total += vertices * (4 + 16) + (vertices * (3 + 4) if outputs == "everything" else 0)
    if outputs in ("everything", "triangles"):
        total += 2 * lattice + 12 * triangles
    return total


def child(a):
    import adcensus_amd as A
    from adcensus_amd import workloads
    from tests import mesh_ref as R
    L = A.lib()
    hip = C.CDLL("libamdhip64.so")
    L.adc_get_stream.restype = C.c_void_p
    L.adc_get_stream.argtypes = [C.c_void_p]
    out = {"version": L.adc_version().decode()}
    st = A.ADCensusStereo(device=0)
    assert st.Initialize(W, H, A.ADCensusOption(max_disparity=D)), A.last_error()
    stream = C.c_void_p(L.adc_get_stream(st._h))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    dm, di, dv, dvi, dt, dc = (L.adc_device_malloc(s) for s in (4 * N, 3 * N, 16 * N, 4 * N, 24 * N, 8))
    ca, cb = L.adc_device_malloc(32 * N), L.adc_device_malloc(32 * N)
    done = {}
    for label, name, max_diff in MAPS:
        if name not in done:
            left, right = workloads.structured_pair(W, H, D, seed=777) if name == "structured" else workloads.noise_pair(W, H, 12345)
            done[name] = (st.match(left, right), left)
        disp, left = done[name]
        assert L.adc_memcpy_h2d(dm, disp.ctypes.data, disp.nbytes) == 0 and L.adc_memcpy_h2d(di, left.ctypes.data, left.nbytes) == 0
        for step in STEPS:
            params = A.MeshParams(max_diff, step)
            want = R.mesh(disp, CALIB, max_diff, step)[3]
            lattice = ((W - 1) // step + 1) * ((H - 1) // step + 1)
            for oname in OUTPUTS:
                every, vtx, tri = oname == "everything", oname != "triangles", oname != "vertices"
                best = 1e9
                for _ in range(a.reps + 1):  # (the first one warms up)
                    assert hip.hipEventRecord(ev0, stream) == 0
                    assert st.mesh_device(dm, CALIB, params, di if every else None, dv if vtx else None, N, dvi if every else None, dt if tri else None, 2 * N,
                                          dc if every else None), A.last_error()
                    assert hip.hipEventRecord(ev1, stream) == 0
                    assert st.wait(), A.last_error()
                    ms = C.c_float(0)
                    assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
                    best = min(best, float(ms.value))
                rep = st.mesh_report()
                assert [getattr(rep, k) for k in R.REPORT_FIELDS] == R.report_words(want), (label, step, oname)
                total = priced_bytes(lattice, rep.vertices, rep.triangles, oname)
                key = "%s s%d %s" % (label, step, oname)
                out[key] = best
                out[key + " bytes"] = total
                out[key + " copy"] = float(L.adc_device_copy_kernel_ms(cb, ca, total // 32 * 16, 5))  # (whole 16-byte words)
            out["%s s%d counts" % (label, step)] = [lattice] + R.report_words(want)
    for b in (dm, di, dv, dvi, dt, dc, ca, cb):
        L.adc_device_free(b)
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_timing.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = os.path.abspath(__file__)
    md = ["# Triangle mesh from a disparity map: timing on one MI355X, 1920x1080", "",
          "`tools/mesh_timing.py`; the final maps of the benchmark's structured and noise pairs (D = 128) with a calibration; one call (`adc_mesh_device`: the "
          "cleared report words, `k_mesh_measure`, `k_mesh_scan`, `k_mesh_emit`, the pinned read-back) between two HIP events on the handle's stream, best of "
          "%d after a warm-up, ms per call.  Bytes priced: 4 per lattice point (the map, read by the measure) + 40 per chunk of 64 lattice points (used word and "
          "two counts: written, scanned, read) + per vertex 4 (the map again) + 16 (the record), with `everything` also 3 (colour) + 4 (vertex_index) + per "
          "triangle 12 + 2 per lattice point (the code byte, written and read) when triangles are asked for.  Copy kernel: `adc_device_copy_kernel_ms` moving "
          "the same bytes (a copy of half of them, read + write)." % a.reps, ""]
    calls = run_child([sys.executable, me, "--child", "calls", "--reps", str(a.reps)], "", 900, TAG)
    md += ["| map, max_diff | step | lattice | vertices | triangles | outputs | MB priced | ms per call | GB/s | copy kernel, same bytes, ms | call / copy |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for label, _, max_diff in MAPS:
        for step in STEPS:
            counts = calls["%s s%d counts" % (label, step)]
            for oname in OUTPUTS:
                key = "%s s%d %s" % (label, step, oname)
                t, total, c = calls[key], calls[key + " bytes"], calls[key + " copy"]
                md.append("| %s, %g | %d | %d | %d | %d | %s | %.1f | %.4f | %.0f | %.4f | %.2f |" % (label, max_diff, step, counts[0], counts[2], counts[3], oname, total / 1e6, t,
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
