"""Builds the shared libraries in-tree (solstrale-rust_amd/_build/):

  libsolstrale_hip.so   hand-written HIP for gfx950 + the C ABI of include/solstrale_hip.h   (hipcc)
  libsolstrale_host.so  C++ host mirror of the reference's Scene / ray_trace surface          (g++)
  profiling             the reference's profiling binary on the device path, native (examples/) (g++)

hipcc cross-compiles gfx950 code objects without a GPU. -ffp-contract=off keeps the device arithmetic the plain
IEEE sequence the parity tests pin (DESIGN.md "fp32 arithmetic contract"). Translation units are compiled in
parallel to objects (only the stale ones) and linked; `build(out_dir=..., extra_hip_flags=...)` makes an A/B variant
of the device library elsewhere (tests/tools/variants.py), selected at run time through SOLSTRALE_BUILD_DIR.
`build_ab()` makes _build_ab/: the same library plus the measured-and-rejected render-kernel variants (-DSOL_AB_KERNELS +
csrc/sol_wavefront.hip: the two wavefront kernels; csrc/sol_pool.hip: the pool kernel; csrc/sol_launch_ab.cpp: their launches), which the product library does not carry. Rejected experiments are not kept in the sources: their records
are profiles/*_ab.txt and the git history.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

HIP_SRC = ["csrc/sol_render.hip", "csrc/sol_aux.hip", "csrc/sol_build.hip", "csrc/sol_api.cpp", "csrc/sol_create.cpp",
           "csrc/sol_launch.cpp", "csrc/sol_post.cpp", "csrc/sol_comm.cpp", "csrc/sol_adaptive.hip", "csrc/sol_envmap.hip", "csrc/sol_lights.hip",
           "csrc/sol_denoise.hip", "csrc/sol_query.hip", "csrc/sol_camera.hip", "csrc/sol_camera.cpp",
           "csrc/sol_geometry.hip", "csrc/sol_geometry.cpp", "csrc/sol_radiance.hip", "csrc/sol_visibility.hip",
           "csrc/sol_lightmap.hip", "csrc/sol_lightmap.cpp", "csrc/sol_lightmap_filter.hip", "csrc/sol_lightmap_filter.cpp", "csrc/sol_lightmap_filter_var.hip", "csrc/sol_lightmap_filter_var.cpp",
           "csrc/sol_gather.cpp", "csrc/sol_gather_adaptive.hip", "csrc/sol_gather_adaptive.cpp",
           "csrc/sol_volume.hip", "csrc/sol_volume.cpp",
           "csrc/sol_depth.hip", "csrc/sol_depth.cpp",
           "csrc/sol_lightmap_sample.hip", "csrc/sol_lightmap_sample.cpp",
           "csrc/sol_lightmap_sh.hip", "csrc/sol_lightmap_sh.cpp",
           "csrc/sol_lightmap_mips.hip", "csrc/sol_lightmap_mips.cpp",
           "csrc/sol_lightmap_charts.hip", "csrc/sol_lightmap_charts.cpp",
           "csrc/sol_lightmap_unwrap.hip", "csrc/sol_lightmap_unwrap.cpp"]
HIP_HDR = ["csrc/sol_types.h", "csrc/sol_math.h", "csrc/sol_trace.h", "csrc/sol_shade.h", "csrc/sol_path.h", "csrc/sol_launch.h",
           "csrc/sol_tree.h", "csrc/sol_build.h", "csrc/sol_scene.h", "csrc/sol_camera.h", "csrc/sol_triangle.h", "csrc/sol_primitive.h", "csrc/sol_geometry.h", "csrc/sol_quant.h", "csrc/sol_wide.h", "csrc/sol_proof.h", "csrc/sol_ray.h", "csrc/sol_wave.h",
           "csrc/sol_sh.h", "csrc/sol_radiance_body.h", "csrc/sol_lightmap.h", "csrc/sol_lightmap_filter.h", "csrc/sol_lightmap_filter_var.h", "csrc/sol_gather.h", "csrc/sol_stage.h", "csrc/sol_bake_checks.h", "csrc/sol_gather_adaptive.h", "csrc/sol_volume.h", "csrc/sol_depth.h", "csrc/sol_lightmap_sample.h", "csrc/sol_lightmap_lookup.h", "csrc/sol_lightmap_sh.h", "csrc/sol_lightmap_mips.h", "csrc/sol_lightmap_charts.h", "csrc/sol_lightmap_unwrap.h", "../include/solstrale_hip.h"]
HOST_SRC = ["host/solstrale_host.cpp", "host/solstrale_obj.cpp", "host/solstrale_host_c.cpp"]
HOST_DEPS = HOST_SRC + ["host/solstrale.hpp", "../include/solstrale_hip.h", "../include/solstrale_host.h"]
EXAMPLES = ["examples/profiling.cpp"]  # native programs over the C++ host mirror (the reference's src/bin/profiling.rs); no Python, no torch

# -packed-fp32-ops (target feature OFF): hipcc otherwise pairs fp32 multiplies and adds into v_pk_mul_f32 / v_pk_add_f32 /
# v_pk_fma_f32 wherever it finds two alike (cross products of the triangle test, shading vectors). On MI355X a packed instruction
# issues like two (4.8 cycles: tests/tools/micro/valu_ops.hip) and its operands must sit in aligned register pairs: the render
# kernel paid for the pairing in moves and in its only 6 VGPR spills. Without them: 0 spills, C1 -5.9 %, C2 -4.8 %, C3 -3.5 %
# (profiles/r03_no_packed_fp32_ab.txt); the arithmetic is the same IEEE operations either way (every frame CRC identical).
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
             "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", "-Wall", "-Wno-unused-value"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(os.path.join(HERE, d)) > t for d in deps)


def _run(cmd):
    print("+", " ".join(cmd), file=sys.stderr, flush=True)  # (never stdout: bench.py's stdout is ONE JSON line)
    subprocess.check_call(cmd, cwd=HERE, stdout=sys.stderr)


def build(force=False, extra_hip_flags=(), out_dir=None, ab_kernels=False):
    """Product library into _build/ (or a variant into out_dir). ab_kernels: the A/B build that also carries the two wavefront
    render kernels and the pool kernel (-DSOL_AB_KERNELS + sol_wavefront.hip, sol_pool.hip, sol_launch_ab.cpp; `build_ab()` puts it into _build_ab/) - the product has one family."""
    out_dir = out_dir or BUILD
    os.makedirs(out_dir, exist_ok=True)
    hip_lib = os.path.join(out_dir, "libsolstrale_hip.so")
    host_lib = os.path.join(out_dir, "libsolstrale_host.so")
    flags_file = os.path.join(out_dir, "hip_flags.txt")
    flags = HIP_FLAGS + (["-DSOL_AB_KERNELS"] if ab_kernels else []) + list(extra_hip_flags)
    sources = HIP_SRC + (["csrc/sol_wavefront.hip", "csrc/sol_pool.hip", "csrc/sol_launch_ab.cpp"] if ab_kernels else [])
    want = " ".join(flags + sources)
    have = open(flags_file).read() if os.path.exists(flags_file) else None
    if have != want:
        force = True
        if have is not None:
            os.remove(flags_file)  # (written again only after a successful link: an interrupted build starts over)
    jobs, objs = [], []
    for src in sources:
        obj = os.path.join(out_dir, os.path.basename(src) + ".o")
        objs.append(obj)
        if force or _stale(obj, [src] + HIP_HDR + ["build.py"]):
            jobs.append([HIPCC] + flags + ["-c", src, "-o", obj])
    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as ex:
            list(ex.map(_run, jobs))
    # link whenever an object is newer than the library (also after a failed or interrupted link of an earlier run)
    if jobs or not os.path.exists(hip_lib) or any(os.path.getmtime(o) > os.path.getmtime(hip_lib) for o in objs):
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", hip_lib, "-ldl"])
    if force or have != want:  # (only when something was built, and atomically: ranks of one job may call build() side by side)
        tmp = flags_file + f".{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            f.write(want)
        os.replace(tmp, flags_file)
    if force or _stale(host_lib, HOST_DEPS + ["build.py"]) or os.path.getmtime(hip_lib) > os.path.getmtime(host_lib):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-pthread"] + HOST_SRC +
             ["-o", host_lib, "-L" + out_dir, "-lsolstrale_hip", "-Wl,-rpath,$ORIGIN"])
    for src in EXAMPLES:
        exe = os.path.join(out_dir, os.path.splitext(os.path.basename(src))[0])
        if force or _stale(exe, [src, "host/solstrale.hpp", "build.py"]) or os.path.getmtime(host_lib) > os.path.getmtime(exe):
            _run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread", src, "-o", exe, "-L" + out_dir, "-lsolstrale_host", "-lsolstrale_hip",
                  "-Wl,-rpath,$ORIGIN"])
    return hip_lib, host_lib


BUILD_AB = os.path.join(HERE, "_build_ab")


def build_ab(force=False):
    return build(force=force, out_dir=BUILD_AB, ab_kernels=True)


BUILD_SAN = os.path.join(HERE, "_build_san")
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


def build_sanitized():
    """_build_san/: the three libraries with AddressSanitizer + UndefinedBehaviorSanitizer on their HOST code (CPU build only: device code
    is not instrumented - no GPU sanitizer runs on this pool). One compiler (hipcc's clang) for all three so that one sanitizer
    runtime serves the process; tests/tools/sanitize.sh runs the CPU suites under it with the runtime preloaded."""
    os.makedirs(BUILD_SAN, exist_ok=True)
    clang = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "lib", "llvm", "bin", "clang++")
    hip_lib = os.path.join(BUILD_SAN, "libsolstrale_hip.so")
    flags = [f for f in HIP_FLAGS if f != "-O3"] + SAN_FLAGS + ["-fno-gpu-sanitize"]
    jobs, objs = [], []
    for src in HIP_SRC:
        obj = os.path.join(BUILD_SAN, os.path.basename(src) + ".o")
        objs.append(obj)
        if _stale(obj, [src] + HIP_HDR + ["build.py"]):
            jobs.append([HIPCC] + flags + ["-c", src, "-o", obj])
    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as ex:
            list(ex.map(_run, jobs))
    if jobs or not os.path.exists(hip_lib):
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-shared-libsan"] + SAN_FLAGS + ["-fno-gpu-sanitize"] + objs + ["-o", hip_lib, "-ldl"])
    host_lib = os.path.join(BUILD_SAN, "libsolstrale_host.so")
    if _stale(host_lib, HOST_DEPS + ["build.py"]) or os.path.getmtime(hip_lib) > os.path.getmtime(host_lib):
        _run([clang, "-std=c++17", "-fPIC", "-shared", "-shared-libsan", "-Wall", "-Wextra", "-pthread"] + SAN_FLAGS + HOST_SRC +
             ["-o", host_lib, "-L" + BUILD_SAN, "-lsolstrale_hip", "-Wl,-rpath,$ORIGIN"])
    for src in EXAMPLES:
        exe = os.path.join(BUILD_SAN, os.path.splitext(os.path.basename(src))[0])
        if _stale(exe, [src, "host/solstrale.hpp", "build.py"]) or os.path.getmtime(host_lib) > os.path.getmtime(exe):
            _run([clang, "-std=c++17", "-shared-libsan", "-Wall", "-Wextra", "-pthread"] + SAN_FLAGS + [src, "-o", exe, "-L" + BUILD_SAN, "-lsolstrale_host",
                  "-lsolstrale_hip", "-Wl,-rpath,$ORIGIN"])
    oracle_lib = os.path.join(BUILD_SAN, "liboracle.so")
    odir = os.path.join(os.path.dirname(HERE), "oracle")
    if not os.path.exists(oracle_lib) or any(os.path.getmtime(os.path.join(odir, f)) > os.path.getmtime(oracle_lib) for f in ("oracle.cpp", "oracle.h")):
        _run([clang, "-std=c++17", "-fPIC", "-shared", "-shared-libsan", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-pthread"] + SAN_FLAGS +
             [os.path.join(odir, "oracle.cpp"), "-o", oracle_lib])
    return BUILD_SAN


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        print(build_sanitized())
        sys.exit(0)
    build(force="--force" in sys.argv)
    if "--ab" in sys.argv:
        build_ab(force="--force" in sys.argv)
