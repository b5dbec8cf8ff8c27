"""Build the native code of this repository (in-tree, gfx950 only).

  csrc/*.hip          -> csrc/libmvs_viewsel.so   (hipcc --offload-arch=gfx950; the product: the kernels k_*.hip (k_tone.hip: tone mapping `gamma` and its host twin) / scan.hip and the host side
                                                  api.hip (contexts, scene, table), solve.hip (solver loop), oneshot.hip (drop-in calls),
                                                  shard.hip (sharded driver: the entry points; shard_table.hip its cost table, shard_plan.hip its halo plan, shard_transport.hip its two
                                                  halo transports, comm.hip the communicators behind it), readback.hip (words from the device through pinned memory);
                                                  mrf.h (what the MRF solver's k_mrf_setup / k_mrf_sweep / k_mrf_polish.hip share) and
                                                  sort_scan.h (the rocprim two-call idiom), comm.h / shard.h (the communicator interface / what the sharded driver's sources share), rows.h / image_routes.h / view_input.h (the host plumbing of rows f5 - f11 / of the PNG and JPEG routes / of the view inputs) and model_corner.h (a face-list corner as k_model.hip and k_glb.hip read it) are internal headers;
                                                  stash.h / spt_io.h / dc_ranges.h / view_batches.h / shard_lists.h / call_barrier.h / png_io.h are plain host headers, fmt6.h,
                                                  png_rle.h, jpeg_base.h, jpeg_dec.h (the view input route of k_jpegdec.hip), png_dec.h (that of k_pngdec.hip: container, inflate, filters and the host twin), lens.h (row f4's arithmetic: k_prep.hip, k_lens.hip and the host twin), level.h (the pyramid levels of the view input: k_level.hip and the host twin); k_viewmask.hip packs the view masks into keep words for k_prep.hip, dc_counters.h, debug_embed.h and tone.h host-and-device ones, that tests/cpp compiles on their own)
  csrc/mgpu.hip       -> csrc/libmvs_blocks.so    (building blocks of include/mvs_viewsel_blocks.h: the test harness's library, links the product)
  csrc/scene_synth.cpp-> csrc/libmvs_synth.so     (g++; synthetic input producer)
  csrc/dmath_host.cpp -> csrc/libmvs_dmath_host.so(g++; CPU build of dmath.h for the arithmetic unit test)

hipcc cross-compiles without a GPU.  -ffp-contract=off and correctly rounded fp32
divide / sqrt are part of the numerical contract (DESIGN.md "Exactness").
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HIP_SOURCES = ["scan.hip", "k_prep.hip", "k_bvh.hip", "k_kdorder.hip", "k_dc.hip", "k_mrf_setup.hip", "k_mrf_sweep.hip", "k_mrf_polish.hip", "readback.hip", "k_region.hip", "k_mesh.hip", "k_patch.hip", "k_seam.hip", "k_texpatch.hip", "k_localseam.hip", "k_atlas.hip", "k_model.hip", "k_glb.hip", "k_png.hip", "k_jpeg.hip", "k_jpegdec.hip", "k_pngdec.hip", "k_lens.hip", "k_level.hip", "k_viewmask.hip", "k_debug.hip", "k_tone.hip", "k_order.hip", "comm.hip", "shard_plan.hip", "shard_table.hip", "shard_transport.hip", "shard.hip", "api.hip", "solve.hip", "oneshot.hip"]
BLOCKS_SOURCES = ["mgpu.hip"]                       # NOT in the product library
BLOCKS_LIB = os.path.join(CSRC, "libmvs_blocks.so")
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "-fno-fast-math", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]
# per-file additions: the SLP vectoriser packs the ray / triangle arithmetic into v_pk_* operations at the price of ~50
# v_mov shuffles per leaf visit in a kernel that is VALU bound (k_bvh.hip: 66 -> 49 VGPRs, fewer instructions without it)
EXTRA_FLAGS = {"k_bvh.hip": ["-fno-slp-vectorize"]}
LIB = os.path.join(CSRC, "libmvs_viewsel.so")


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _hipcc():
    for c in ("/opt/rocm/bin/hipcc", "hipcc"):
        if os.path.exists(c) or c == "hipcc":
            return c


def build_hip(force=False, verbose=False):
    headers = [os.path.join(CSRC, h) for h in ("ctx.h", "rows.h", "image_routes.h", "view_input.h", "view_batches.h", "sort_scan.h", "mrf.h", "comm.h", "shard.h", "shard_lists.h", "dmath.h", "call_barrier.h", "dc_ranges.h", "dc_counters.h", "stash.h", "spt_io.h", "fmt6.h", "png_io.h", "png_rle.h", "jpeg_base.h", "jpeg_dec.h", "png_dec.h", "lens.h", "level.h", "debug_embed.h", "tone.h", "model_corner.h")] + [os.path.join(HERE, "..", "include", h) for h in ("mvs_viewsel.h", "mvs_viewsel_blocks.h")]
    objs, bobjs, jobs = [], [], []
    for src in HIP_SOURCES + BLOCKS_SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", ".o"))
        (bobjs if src in BLOCKS_SOURCES else objs).append(o)
        if force or _newer(o, [s, os.path.abspath(__file__)] + headers):
            jobs.append([_hipcc()] + HIP_FLAGS + EXTRA_FLAGS.get(src, []) + ["-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    if jobs or force or _newer(LIB, objs):
        run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    if jobs or force or _newer(BLOCKS_LIB, bobjs + [LIB]):
        run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", BLOCKS_LIB] + bobjs + ["-L" + CSRC, "-lmvs_viewsel", "-Wl,-rpath,$ORIGIN"])
    return LIB


def build_host(force=False):
    out = []
    for src, lib in (("scene_synth.cpp", "libmvs_synth.so"), ("dmath_host.cpp", "libmvs_dmath_host.so")):
        s = os.path.join(CSRC, src); l = os.path.join(CSRC, lib)
        if force or _newer(l, [s, os.path.join(CSRC, "dmath.h")]):
            subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-std=c++17",
                                   "-shared", "-o", l, s])
        out.append(l)
    return out


def build_test_tools(force=False):
    """tests/tools/librccl_fake.so: the test double the RCCL communicator of csrc/comm.hip binds when MVS_RCCL_LIB names it (thread-ranks on
    one device; see tests/tools/fake_rccl.hip).  tests/tools/libdc_postprocess_ctx.so: postprocess_face_infos on a context the test owns
    (dc_postprocess_ctx.hip; links the product library).  Test infrastructure: nothing of the product links or loads either by itself."""
    tools = os.path.join(os.path.dirname(HERE), "tests", "tools")
    out = []
    for name, lib, extra in (("fake_rccl.hip", "librccl_fake.so", []), ("dc_postprocess_ctx.hip", "libdc_postprocess_ctx.so", ["-L" + CSRC, "-lmvs_viewsel", "-Wl,-rpath,$ORIGIN/../../mvs-texturing_amd/csrc"])):
        src, lib = os.path.join(tools, name), os.path.join(tools, lib)
        if os.path.exists(src) and (force or _newer(lib, [src] + ([LIB] if extra else []))):
            subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, src] + extra)
        out.append(lib)
    return out


def build_all(force=False, verbose=False):
    return [build_hip(force, verbose)] + build_host(force) + build_test_tools(force)


if __name__ == "__main__":
    print("\n".join(build_all(force="--force" in sys.argv, verbose=True)))
