#!/usr/bin/env python3
"""Build libmmf_hg.so (gfx950) in-tree with hipcc: one object per .hip, then one shared library.

    python multimodal-fusion_amd/csrc/build.py [--force] [-j N]

-ffp-contract=off is part of the numerics contract (include/mmf_hg.h): every fused multiply-add in
the kernels is an explicit fmaf.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
OUT = os.path.join(PKG, "libmmf_hg.so")
OBJ = os.path.join(HERE, "_obj")
SOURCES = ["mmf_api.hip", "mmf_prep.hip", "mmf_scan_f32.hip", "mmf_scan_bf16.hip", "mmf_scan_b16w.hip", "mmf_scan_b16c.hip", "mmf_select.hip", "mmf_edges.hip", "mmf_segments.hip", "mmf_knn_clique.hip", "mmf_direct.hip", "mmf_kmeans.hip", "mmf_order.hip", "mmf_pool.hip", "mmf_stream_stats.hip", "mmf_topk.hip", "mmf_fast_anyk.hip", "mmf_topk_anyk.hip", "mmf_hgconv.hip", "mmf_readout.hip", "mmf_hgpair.hip", "mmf_hg16.hip"]
HEADERS = ["mmf_dev.h", "mmf_host.h", "mmf_rerank_combined.h", "mmf_hgshare.h", os.path.join(ROOT, "include", "mmf_hg.h"), os.path.join(ROOT, "include", "mmf_hg_pool.h"),
           os.path.join(ROOT, "include", "mmf_hg_stream.h"), os.path.join(ROOT, "include", "mmf_hg_topk.h"), os.path.join(ROOT, "include", "mmf_hg_topk16.h"),
           os.path.join(ROOT, "include", "mmf_hg_wide.h"), os.path.join(ROOT, "include", "mmf_hg_wide_seg.h"),
           os.path.join(ROOT, "include", "ext", "mmf_hg_topk16_seg.h"), os.path.join(ROOT, "include", "ext", "mmf_hg_topk_xy.h"),
           os.path.join(ROOT, "include", "ext", "mmf_hg_seg_exact.h"), os.path.join(ROOT, "include", "ext", "mmf_hg_topk_anyk.h"),
           os.path.join(ROOT, "include", "ext", "mmf_hg_kmeans_ragged.h"), os.path.join(ROOT, "include", "ext", "mmf_hg_cross_seg.h"),
           os.path.join(ROOT, "include", "ext", "mmf_hg_cross_seg16.h"), os.path.join(ROOT, "include", "ext", "mmf_hg_cross_segw.h"),
           os.path.join(ROOT, "include", "ext", "mmf_hg_fast_anyk.h"), os.path.join(ROOT, "include", "ext", "mmf_hg_wide_anyk.h"),
           os.path.join(ROOT, "include", "ext", "mmf_hg_seg_anyk.h"), os.path.join(ROOT, "include", "ext", "mmf_hg_cross_seg_anyk.h"),
           os.path.join(ROOT, "include", "ext", "mmf_hg_cross_segw_anyk.h"), os.path.join(ROOT, "include", "ext", "mmf_hg_segw_anyk.h"),
           os.path.join(ROOT, "include", "ext", "mmf_hg_topk16_anyk.h"), os.path.join(ROOT, "include", "ext", "mmf_hg_topk16_xy_anyk.h"),
           os.path.join(ROOT, "include", "ext", "mmf_hg_hgconv.h"), os.path.join(ROOT, "include", "ext", "mmf_hg_readout.h"),
           os.path.join(ROOT, "include", "ext", "mmf_hg_hgpair.h"), os.path.join(ROOT, "include", "ext", "mmf_hg_hg16.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-std=c++17", "-fno-gpu-rdc",
         "-Wall", "-Wno-unused-function"]
# Per-file extras.  Both scans take maxima of MFMA results per tile; without -fno-honor-nans every fmaxf input is
# canonicalised first (v_max x, x): 22 instead of 14 VALU instructions per tile in the 16-bit scan (1-2 % of the
# kernel); together with the out-of-line list path the exact f32 scan went from 54.0 to 49.3 ms at N = 65536 (same-
# process A/B).  Non-finite inputs are outside the numerics contract; infinities are still honoured
# (-inf is the padding bias and the "no key" marker).
EXTRA_FLAGS = {"mmf_scan_bf16.hip": ["-fno-honor-nans"], "mmf_scan_f32.hip": ["-fno-honor-nans"],
               "mmf_scan_b16w.hip": ["-fno-honor-nans"]}


def _newer(target: str, deps) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def build(force: bool = False, jobs: int = 6, verbose: bool = False) -> str:
    os.makedirs(OBJ, exist_ok=True)
    hdrs = [h if os.path.isabs(h) else os.path.join(HERE, h) for h in HEADERS]
    todo = []
    objs = []
    for src in SOURCES:
        sp = os.path.join(HERE, src)
        op = os.path.join(OBJ, src.replace(".hip", ".o"))
        objs.append(op)
        if force or not _newer(op, [sp, *hdrs, os.path.abspath(__file__)]):
            todo.append((sp, op))

    def cc(job):
        sp, op = job
        cmd = [HIPCC, *FLAGS, *EXTRA_FLAGS.get(os.path.basename(sp), []), "-c", sp, "-o", op]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {sp}:\n{r.stdout}\n{r.stderr}")
        if r.stderr.strip() and verbose:
            print(r.stderr)
        return op

    if todo:
        with ThreadPoolExecutor(max_workers=max(1, jobs)) as ex:
            list(ex.map(cc, todo))
    if todo or force or not _newer(OUT, objs):
        cmd = [HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", *objs, "-o", OUT + ".tmp"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
        os.replace(OUT + ".tmp", OUT)
    return OUT


if __name__ == "__main__":
    j = 6
    if "-j" in sys.argv:
        j = int(sys.argv[sys.argv.index("-j") + 1])
    print(build(force="--force" in sys.argv, jobs=j, verbose=True))
