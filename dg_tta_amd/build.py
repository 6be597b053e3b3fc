"""Builds libdgtta_hip.so (gfx950) in-tree with hipcc. No torch dependency; cross-compiles without a GPU."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

CSRC = Path(__file__).resolve().parent / "csrc"
LIB = Path(__file__).resolve().parent / "libdgtta_hip.so"
SOURCES = ["lib.hip", "mind3d.hip", "gin.hip", "warp.hip", "softdice.hip", "dice_ce.hip", "region_loss.hip", "region_map.hip", "adamw.hip", "resample.hip", "window_features.hip",
           "window_logits.hip", "conv_dispatch.hip", "conv_ref.hip", "instnorm.hip", "seghead.hip", "seghead_mfma.hip", "layout_argmax.hip", "conv_mfma.hip",
           "conv_rows.hip", "conv_ring.hip", "conv_wgrad.hip", "conv_wgrad_rows.hip", "conv_wgrad_flat.hip", "conv_wgrad_s2.hip", "conv_wgrad_reduce.hip",
           "conv_wgrad_ring.hip", "convt_wgrad.hip", "head_wgrad.hip", "convt_gemm.hip", "conv_s2.hip", "conv_aniso.hip", "deform.hip", "surface.hip",
           "components.hip", "sgd.hip", "spatial_aug.hip", "intensity_aug.hip", "mirror.hip", "fingerprint.hip"]
# conv_ring.hip: the 64-input-channel step body (432 MFMAs, 192 fragment reads, fully unrolled) is above hipcc's default
# pragma-unroll threshold; partially unrolled its register arrays are indexed dynamically and land in scratch
EXTRA_FLAGS = {"conv_ring.hip": ["-mllvm", "-pragma-unroll-threshold=262144"]}
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]


def source_sha16():
    """sha256 (16 hex) over the kernel sources and the C ABI header: the stamp a profile summary carries, so that a bench line
    can tell whether the profile it quotes was measured on the kernels it is timing."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.h")) + [CSRC.parents[1] / "include" / "dgtta.h"]):
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()[:16]


def _stale(out, deps):
    return (not out.exists()) or any(d.stat().st_mtime > out.stat().st_mtime for d in deps)


def _build(obj_dir, flags, lib, link_flags=(), force=False, verbose=True, capture=False):
    """Compiles every stale source into obj_dir with `flags` (6 at a time) and links `lib` if anything changed."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj_dir.mkdir(parents=True, exist_ok=True)
    hdrs = list(CSRC.glob("*.h")) + [CSRC.parents[1] / "include" / "dgtta.h"]
    objs, jobs = [], []
    for s in SOURCES:
        src, obj = CSRC / s, obj_dir / (s + ".o")
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            jobs.append([hipcc, *flags, *EXTRA_FLAGS.get(s, []), "-c", str(src), "-o", str(obj)])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, capture_output=capture)

    with ThreadPoolExecutor(max_workers=6) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(lib, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *link_flags, "-o", str(lib), *map(str, objs)])
    return lib


def build(force=False, verbose=True):
    return _build(CSRC, FLAGS, LIB, force=force, verbose=verbose)


ASAN_DIR = CSRC.parents[1] / "build" / "asan"
ASAN_FLAGS = ["--offload-arch=gfx950", "-O1", "-g", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
              "-fno-gpu-sanitize", "-fno-omit-frame-pointer", "-Wno-unused-function"]


def build_asan(verbose=False):
    """Host-side sanitizer build of the C-ABI shim: the HOST code of every translation unit (argument
    checks, size queries, launch plans, dispatch) instrumented with AddressSanitizer + UndefinedBehaviorSanitizer, the
    device code left as it is (GPU sanitizers are not available on the pool).  Goes to build/asan/ (git-ignored), never
    into the package: the product always loads dg_tta_amd/libdgtta_hip.so.  tests/test_host_logic.py drives it."""
    return _build(ASAN_DIR, ASAN_FLAGS, ASAN_DIR / "libdgtta_hip_asan.so", ["-fsanitize=address,undefined"], verbose=verbose,
                  capture=not verbose)


if __name__ == "__main__":
    if "--asan" in sys.argv:
        print(build_asan(verbose=True))
    else:
        build(force="--force" in sys.argv)
        print(LIB)
