#!/usr/bin/env python3
"""Times the TSDF volume (adc_tsdf_integrate_device: the cleared report words, k_tsdf_integrate, the pinned read-back;
adc_tsdf_extract_device: the cleared words, k_tsdf_measure, k_tsdf_scan, k_tsdf_emit, the read-back) on one MI355X with 1920x1080 maps,
prices the traffic against the copy kernel and checks that the benchmark's headline did not move; writes profiles/tsdf_timing.md.

    python tools/tsdf_timing.py [--mesh] [--parent-lib DIR/libadcensus_hip.so --parent-commit HASH] [--out profiles/tsdf_timing.md]

The driver starts one child process per step (this file with --child calls, or bench.py for the headline), each with its own time
limit, and stops at the first step that fails.
  calls     per map (the final maps a Match delivers for the benchmark's structured and noise pairs, D = 128), volume (256^3 and 512^3
            voxels spanning the same cube around the map's median depth, truncation 4 voxels) and colour (with the colour volume and the
            left image, without both): one integrate into the EMPTY volume and one into the volume that holds that frame, then one
            extract with room for every point, each between two HIP events on the handle's stream, best of --reps after a warm-up.
            The volume is downloaded once to count the 16-byte groups the frame touches; the bytes priced stand next to the time, and
            next to the time the copy kernel (adc_device_copy_kernel_ms) takes to move the same bytes (a copy of half of them: read +
            write)
  headline  bench.py --gpus 1 of the parent build and of this build (ADC_HIP_LIB selects the library), --reps repetitions each,
            alternating; the new median is judged against the min-max spread of the parent's own repetitions
  mesh      (--mesh; writes profiles/tsdf_mesh_timing.md instead) per map and volume, with the colour volume: one frame fused, then
            adc_tsdf_extract_device and adc_tsdf_mesh_device for the vertices alone, the triangles alone and both, with room for every
            record, each between two HIP events, best of --reps after a warm-up, next to the copy kernel on the bytes priced; then the
            headline as above"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, D = 1920, 1080, 128
N = W * H
CALIB = (0.8 * W, 0.16, W / 2 - 0.3, H / 2 + 0.2, 1.25)
MAPS = ["structured", "noise"]
SIDES = [256, 512]
TAG = "TSDF_TIMING "
ANALYSIS_HEADING = "## What bounds the kernels"  # written by hand below the tables of the output file; kept when the tables are rewritten


def child(a):
    import adcensus_amd as A
    from adcensus_amd import workloads
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
    dm, di, dc = (L.adc_device_malloc(s) for s in (4 * N, 3 * N, 4))
    ca, cb = L.adc_device_malloc(1 << 30), L.adc_device_malloc(1 << 30)
    frame = A.TsdfFrame(CALIB)

    def timed(call):
        best = 1e9
        for _ in range(a.reps + 1):  # (the first one warms up)
            assert hip.hipEventRecord(ev0, stream) == 0
            assert call(), A.last_error()
            assert hip.hipEventRecord(ev1, stream) == 0
            assert st.wait(), A.last_error()
            ms = C.c_float(0)
            assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
            best = min(best, float(ms.value))
        return best

    def copy_ms(total):
        total = min(total, 2 << 30)
        return float(L.adc_device_copy_kernel_ms(cb, ca, total // 32 * 16, 5))  # (whole 16-byte words)

    for name in MAPS:
        left, right = workloads.structured_pair(W, H, D, seed=777) if name == "structured" else workloads.noise_pair(W, H, 12345)
        disp = st.match(left, right)
        assert L.adc_memcpy_h2d(dm, disp.ctypes.data, disp.nbytes) == 0 and L.adc_memcpy_h2d(di, left.ctypes.data, left.nbytes) == 0
        a_ = np.abs(disp)
        ok = np.isfinite(a_) & (a_ + CALIB[4] > 0)
        z = CALIB[0] * CALIB[1] / (a_[ok] + CALIB[4])
        zmed = float(np.median(z))
        extent = 1.25 * zmed  # the image's width at the median depth
        for side in SIDES:
            voxel = extent / side
            for colour in (False, True):
                p = A.TsdfParams(side, side, side, voxel, (-extent / 2, -extent / 2, zmed - extent / 2), 4 * voxel, max_weight=64, flags=A.TSDF_COLOR if colour else 0)
                assert st.tsdf_create(p), A.last_error()
                img = di if colour else None
                key = "%s %d %s" % (name, side, "colour" if colour else "plain")

                def first():
                    return st.tsdf_reset() and st.tsdf_integrate_device(dm, frame, img)

                def reset_only():
                    return st.tsdf_reset()

                t_first = timed(first) - timed(reset_only)      # (the reset's memsets are timed alone and taken off)
                t_again = timed(lambda: st.tsdf_integrate_device(dm, frame, img))
                rep = st.tsdf_report()[0]
                tsdf, _ = st.tsdf_download()
                groups = int((tsdf.reshape(-1, 4) >> 16).any(axis=1).sum())
                del tsdf
                cap = 3 * side ** 3 // 8
                dp = L.adc_device_malloc(16 * cap)
                t_ext = timed(lambda: st.tsdf_extract_device(dp, cap, None, dc))
                xrep = st.tsdf_report()[1]
                assert xrep.points <= cap
                L.adc_device_free(dp)
                vox = side ** 3
                ibytes = groups * 32 * (2 if colour else 1) + 4 * N + (3 * N if colour else 0)
                # extract: the voxel words once per launch that walks them (measure, emit), the +y / +z neighbours of the seen voxels
                # from cache, the tile counts written, scanned and read, the records
                xbytes = 2 * 4 * vox + 3 * 4 * (vox // 256) + 16 * xrep.points + (8 * xrep.points if colour else 0)
                out[key] = dict(voxel=voxel, zmed=zmed, first=t_first, again=t_again, extract=t_ext, report=[rep.in_frustum, rep.no_depth, rep.occluded, rep.updated],
                                groups=groups, seen=xrep.voxels_seen, points=xrep.points, ibytes=ibytes, xbytes=xbytes, icopy=copy_ms(ibytes), xcopy=copy_ms(xbytes))
                print(key, out[key], flush=True)
        assert st.tsdf_destroy()
    for b in (dm, di, dc, ca, cb):
        L.adc_device_free(b)
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.Release()
    print(TAG + json.dumps(out), flush=True)


def child_mesh(a):
    import adcensus_amd as A
    from adcensus_amd import workloads
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
    dm, di, dc = (L.adc_device_malloc(s) for s in (4 * N, 3 * N, 8))
    ca, cb = L.adc_device_malloc(1 << 30), L.adc_device_malloc(1 << 30)
    frame = A.TsdfFrame(CALIB)

    def timed(call):
        best = 1e9
        for _ in range(a.reps + 1):  # (the first one warms up)
            assert hip.hipEventRecord(ev0, stream) == 0
            assert call(), A.last_error()
            assert hip.hipEventRecord(ev1, stream) == 0
            assert st.wait(), A.last_error()
            ms = C.c_float(0)
            assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
            best = min(best, float(ms.value))
        return best

    def copy_ms(total):
        total = min(total, 2 << 30)
        return float(L.adc_device_copy_kernel_ms(cb, ca, total // 32 * 16, 5))  # (whole 16-byte words)

    for name in MAPS:
        left, right = workloads.structured_pair(W, H, D, seed=777) if name == "structured" else workloads.noise_pair(W, H, 12345)
        disp = st.match(left, right)
        assert L.adc_memcpy_h2d(dm, disp.ctypes.data, disp.nbytes) == 0 and L.adc_memcpy_h2d(di, left.ctypes.data, left.nbytes) == 0
        a_ = np.abs(disp)
        ok = np.isfinite(a_) & (a_ + CALIB[4] > 0)
        zmed = float(np.median(CALIB[0] * CALIB[1] / (a_[ok] + CALIB[4])))
        extent = 1.25 * zmed  # the image's width at the median depth
        for side in SIDES:
            voxel = extent / side
            p = A.TsdfParams(side, side, side, voxel, (-extent / 2, -extent / 2, zmed - extent / 2), 4 * voxel, max_weight=64, flags=A.TSDF_COLOR)
            assert st.tsdf_create(p), A.last_error()
            assert st.tsdf_integrate_device(dm, frame, di) and st.wait(), A.last_error()
            assert st.tsdf_mesh_device(dc, 0, dc, 0) and st.wait(), A.last_error()  # (counts only)
            rep = st.tsdf_mesh_report()
            nv, nt = rep.vertices, rep.triangles
            dv, dt = L.adc_device_malloc(16 * max(nv, 1)), L.adc_device_malloc(12 * max(nt, 1))
            t = dict(extract=timed(lambda: st.tsdf_extract_device(dv, nv, None, dc)), vertices=timed(lambda: st.tsdf_mesh_device(dv, nv, None, 0, None, dc)),
                     triangles=timed(lambda: st.tsdf_mesh_device(None, 0, dt, nt, None, dc)), both=timed(lambda: st.tsdf_mesh_device(dv, nv, dt, nt, None, dc)),
                     count=timed(lambda: st.tsdf_mesh_device(dc, 0, dc, 0, None, dc)))
            assert st.tsdf_mesh_report().triangles == nt and st.tsdf_report()[1].points == nv
            L.adc_device_free(dv)
            L.adc_device_free(dt)
            vox, tiles = side ** 3, side ** 3 // 256
            # a pass over the volume reads its words once (the rows above and behind come from cache); a tile's two counts are written,
            # scanned (read + written) and read; a vertex record is 16 bytes and reads two colour words; a first rank is written per
            # voxel that owns a crossing (at most one per vertex) and read, with up to three voxel words, per triangle corner
            xbytes = 2 * 4 * vox + 12 * tiles + 24 * nv
            b = dict(extract=xbytes, count=4 * vox + 2 * 12 * tiles, vertices=2 * 4 * vox + 2 * 12 * tiles + 24 * nv,
                     triangles=3 * 4 * vox + 2 * 12 * tiles + 4 * nv + (12 + 48) * nt, both=3 * 4 * vox + 2 * 12 * tiles + 28 * nv + (12 + 48) * nt)
            key = "%s %d" % (name, side)
            out[key] = dict(voxel=voxel, report=[rep.voxels_seen, rep.vertices, rep.triangles, rep.cells_seen, rep.cells_surface], ms=t, bytes=b,
                            copy={k: copy_ms(v) for k, v in b.items()})
            print(key, out[key], flush=True)
        assert st.tsdf_destroy()
    for buf in (dm, di, dc, ca, cb):
        L.adc_device_free(buf)
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.Release()
    print(TAG + json.dumps(out), flush=True)


def mesh_tables(a, me):
    md = ["# Triangle mesh of the TSDF volume: timing on one MI355X, 1920x1080 maps", "",
          "`tools/tsdf_timing.py --mesh`; the volumes of profiles/tsdf_timing.md (the final maps of the benchmark's structured and noise pairs, D = 128, the identity "
          "pose; cubes of 256^3 and 512^3 voxels around the map's median depth, truncation 4 voxels, a colour volume) after ONE fused frame.  One call between "
          "two HIP events on the handle's stream, with room for every record, best of %d after a warm-up, ms per call; `adc_tsdf_extract_device` on the same "
          "volume in the same run.  Bytes priced: 4 per voxel and pass over the volume (measure; vertex pass; triangle pass), 24 per tile of 256 voxels (two "
          "counts: written, scanned, read), 24 per vertex record (28 when its first rank is written), 60 per triangle (its record, and per corner a rank and up "
          "to three voxel words).  Copy kernel: `adc_device_copy_kernel_ms` moving the same bytes (a copy of half of them, read + write)." % a.reps, ""]
    calls = run_child([sys.executable, me, "--child", "mesh", "--reps", str(a.reps)], "", 1000, TAG)
    md += ["| map | volume | voxels seen | vertices | triangles | cells seen | surface cells |", "|---|---|---|---|---|---|---|"]
    for name in MAPS:
        for side in SIDES:
            c = calls["%s %d" % (name, side)]
            md.append("| %s | %d^3 | %d | %d | %d | %d | %d |" % ((name, side) + tuple(c["report"])))
    md += ["", "| map | volume | call | MB priced | ms per call | GB/s | copy kernel, same bytes, ms | call / copy |", "|---|---|---|---|---|---|---|---|"]
    for name in MAPS:
        for side in SIDES:
            c = calls["%s %d" % (name, side)]
            for k, label in (("extract", "adc_tsdf_extract_device"), ("count", "mesh, counts only"), ("vertices", "mesh, vertices only"), ("triangles", "mesh, triangles only"),
                             ("both", "mesh, both")):
                md.append("| %s | %d^3 | %s | %.1f | %.4f | %.0f | %.4f | %.2f |" % (name, side, label, c["bytes"][k] / 1e6, c["ms"][k], c["bytes"][k] / c["ms"][k] / 1e6,
                                                                                     c["copy"][k], c["ms"][k] / c["copy"][k] if c["copy"][k] > 0 else float("nan")))
    return md


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
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_timing.md"))
    a = ap.parse_args()
    if a.child:
        return child_mesh(a) if a.child == "mesh" else child(a)
    me = os.path.abspath(__file__)
    if a.mesh and a.out == os.path.join(ROOT, "profiles", "tsdf_timing.md"):
        a.out = os.path.join(ROOT, "profiles", "tsdf_mesh_timing.md")
    md = mesh_tables(a, me) if a.mesh else tsdf_tables(a, me)
    md += ["", "## The benchmark's headline against the parent (%s), %d alternating repetitions each" % (a.parent_commit, a.reps), ""]
    md += headline(a)
    text = "\n".join(md) + "\n"
    # the hand-written analysis behind the tables (everything from its heading on) survives a new measurement
    if os.path.exists(a.out):
        old = open(a.out).read()
        at = old.find(ANALYSIS_HEADING)
        if at >= 0:
            text += "\n" + old[at:]
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


def tsdf_tables(a, me):
    md = ["# TSDF volume: timing on one MI355X, 1920x1080 maps", "",
          "`tools/tsdf_timing.py`; the final maps of the benchmark's structured and noise pairs (D = 128) with a calibration, the identity pose; cubes of 256^3 and "
          "512^3 voxels around the map's median depth whose side is the image's width at that depth, truncation 4 voxels.  One call between two HIP events on the "
          "handle's stream, best of %d after a warm-up, ms per call.  `first` fuses the frame into the empty volume (the time of the reset in front of it is "
          "measured alone and taken off), `again` into the volume that already holds it.  Bytes priced for integrate: 32 per touched 16-byte group of voxel words "
          "(read + write; as much again for the colour words) + the map (4 per pixel) and the image (3 per pixel); for extract: the voxel words read by the "
          "measure and by the emit (8 per voxel), 12 per tile of 256 voxels (its count: written, scanned, read), 16 per record (24 with colours).  Copy kernel: "
          "`adc_device_copy_kernel_ms` moving the same bytes (a copy of half of them, read + write)." % a.reps, ""]
    calls = run_child([sys.executable, me, "--child", "calls", "--reps", str(a.reps)], "", 1000, TAG)
    md += ["## adc_tsdf_integrate_device", "",
           "| map | volume | colour | voxel | in frustum | updated | touched groups | MB priced | first, ms | again, ms | Gvoxel/s (again) | copy kernel, same bytes, ms | again / copy |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in MAPS:
        for side in SIDES:
            for colour in ("plain", "colour"):
                c = calls["%s %d %s" % (name, side, colour)]
                md.append("| %s | %d^3 | %s | %.5f | %d | %d | %d | %.1f | %.4f | %.4f | %.1f | %.4f | %.1f |" % (
                    name, side, colour, c["voxel"], c["report"][0], c["report"][3], c["groups"], c["ibytes"] / 1e6, c["first"], c["again"], side ** 3 / c["again"] / 1e6,
                    c["icopy"], c["again"] / c["icopy"] if c["icopy"] > 0 else float("nan")))
    md += ["", "## adc_tsdf_extract_device", "",
           "| map | volume | colour | voxels seen | points | MB priced | ms per call | GB/s | copy kernel, same bytes, ms | call / copy |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name in MAPS:
        for side in SIDES:
            for colour in ("plain", "colour"):
                c = calls["%s %d %s" % (name, side, colour)]
                md.append("| %s | %d^3 | %s | %d | %d | %.1f | %.4f | %.0f | %.4f | %.2f |" % (
                    name, side, colour, c["seen"], c["points"], c["xbytes"] / 1e6, c["extract"], c["xbytes"] / c["extract"] / 1e6, c["xcopy"],
                    c["extract"] / c["xcopy"] if c["xcopy"] > 0 else float("nan")))
    return md


def headline(a):
    md = []
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
    return md


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
