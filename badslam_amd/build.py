"""Builds libbadslam_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libbadslam_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# -ffp-contract=off + correctly rounded fp32 divide/sqrt: the association predicates must round
# exactly like the CPU oracle's (bit-exact integer outputs); see DESIGN.md "Numerics".
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function", "-Wno-pass-failed"]
# -fno-slp-vectorize: v_pk_{mul,add,fma}_f32 issue at half rate on gfx950 (measured, tools/microbench_valu.hip), so
# SLP-packed fp32 gains nothing and costs v_mov packing + ~40 % more VGPRs; pose kernel -19 %, see DESIGN.md.


def sources():
    """The translation unit of the project's kernels (what tools/kernel_regs.py and tools/isa_stats.py look at)."""
    return [os.path.join(CSRC, "badslam_hip.hip")]


def library_sources():
    """... and the one that only wraps a rocPRIM call, kept apart so that it leaves the device code of the first alone."""
    return sources() + [os.path.join(CSRC, "mesh_sort.hip")]


def needs_build():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "badslam_hip.h")]
    return any(os.path.getmtime(d) > t for d in deps)


HOST = os.path.join(HERE, "host")
HOST_SO = os.path.join(HERE, "libbadslam_host.so")
# host-only C++ (DirectBA loops); no device code, links the kernel library by $ORIGIN rpath
HOST_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__",
              "-I/opt/rocm/include", "-L" + HERE, "-lbadslam_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"]


def needs_host_build():
    if not os.path.exists(HOST_SO):
        return True
    t = os.path.getmtime(HOST_SO)
    deps = [os.path.join(HOST, f) for f in os.listdir(HOST)] + [os.path.join(HERE, "..", "include", "badslam_hip.h"), SO]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    if force or needs_build():
        cmd = [HIPCC] + FLAGS + library_sources() + ["-o", SO]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
    if force or needs_host_build():
        cmd = ["g++"] + [os.path.join(HOST, f) for f in ("direct_ba.cpp", "io.cpp", "pairwise_frame_tracking.cpp", "bad_slam.cpp", "rectification.cpp", "pose_graph.cpp", "loop_closure.cpp", "place_recognition.cpp", "c_api.cpp")] + HOST_FLAGS + ["-lz", "-o", HOST_SO]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
    return SO


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    print(SO)
