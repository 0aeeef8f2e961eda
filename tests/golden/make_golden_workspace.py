#!/usr/bin/env python3
"""Record every *_workspace_bytes query of the built library over a grid of arguments into workspace_sizes.json (data only):
{query: [[args, bytes], ...]}.  Callers may cache these sizes, so tests/test_host_cpu.py holds every later library to them.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_workspace.py

The grid has, per query, the arguments that answer 0 (zero, negative, over the limit), 1, both sides of every threshold of its
formula, and the production shapes.  cmdiad_ocsvm_fit_workspace_bytes is left out: its hipcub term depends on whether a device
is visible."""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from cmdiad_amd import _native as nat  # noqa: E402

XYZ_ROWS, RGB_ROWS = 76518, 19129                      # the bench libraries
FPS_TIER = 512 * 56 + 9728                             # register + LDS tiers of fps_ragged_kernel
SORT_TILE, PLAN_THREADS = 4096, 1024                   # kSortTile, kPlanThreads
ROWS = [0, -1, 1, 15, 16, 17, 127, 128, 129, 300, 100, 2048, 16 * 8 * 256 - 1, 16 * 8 * 256, 16 * 8 * 256 + 1, RGB_ROWS, XYZ_ROWS]
SIDES = [(0, 5), (5, 0), (-1, 7), (1, 1), (5, 7), (17, 19), (33, 31), (9, 300), (300, 11), (224, 224), (800, 800), (16384, 16384),
         (16385, 4), (4, 16385), (8192, 4096)]
IMAGES = [-1, 0, 1, 2, 32, 65535, 65536]


def product(*axes):
    return [list(a) for a in itertools.product(*axes)]


GRID = {
    "cmdiad_gemm_streamk_workspace_bytes": [[]],
    "cmdiad_fps_workspace_bytes": product([-1, 0, 1, 2, 32], [-1, 0, 1, 1024, 28672, 28673, FPS_TIER - 1, FPS_TIER, FPS_TIER + 1, 50176]),
    "cmdiad_reweight_workspace_bytes": product([0, 1, 32], ROWS),
    "cmdiad_reweight_pair_workspace_bytes": product(ROWS, [1, 100, 16 * 8 * 256 + 1, RGB_ROWS]),
    "cmdiad_coreset_workspace_bytes": product([-1, 0, 1, 3, 4, 5, 70, 127, 128, 129, XYZ_ROWS, 765184], [0, 1, 2, 32, 126, 768, 1024],
                                              [-1, 0, 1, 8, 7651]),
    "cmdiad_coreset_f32_workspace_bytes": product([-1, 0, 1, 3, 4, 5, 70, 127, 128, 129, XYZ_ROWS, 765184], [0, 1, 2, 32, 63, 768, 1024],
                                                  [-1, 0, 1, 8, 7651]),
    "cmdiad_rows_dedup_workspace_bytes": [[q] for q in (-5, 0, 1, 15, 16, 17, PLAN_THREADS - 1, PLAN_THREADS, PLAN_THREADS + 1, PLAN_THREADS + 5,
                                                        2 * PLAN_THREADS, 2 * PLAN_THREADS + 1, 3136, 100352)],
    "cmdiad_knn_workspace_bytes": product([-1, 0, 1, 2, 32], [-1, 0, 1, 2047, 2048, 2049, 50176]),
    "cmdiad_interp3nn_workspace_bytes": product([-1, 0, 1, 2, 32], [-1, 0, 1, 63, 64, 65, 128, 3226, 4096]),
    "cmdiad_transformer_block_workspace_bytes": [[0, 768, 3072], [-1, 768, 3072], [197, 0, 3072], [197, 768, 0], [197, -64, 3072], [1, 64, 1],
                                                 [65, 128, 512], [255, 384, 1536], [256, 384, 1536], [257, 384, 1536], [197, 768, 3072],
                                                 [25120, 768, 3072], [32768, 384, 1536], [100352, 768, 3072]],
    "cmdiad_plane_ransac_workspace_bytes": [[i] for i in (-1, 0, 1, 16, 1000, 1 << 20, (1 << 20) + 1)],
    "cmdiad_dbscan_workspace_bytes": [[n] for n in (-1, 0, 1, 29, 500, 2047, 2048, 2049, 65536, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 640000,
                                                    1 << 24, (1 << 24) + 1)],
    "cmdiad_scan_edges_workspace_bytes": [list(s) for s in SIDES],
    "cmdiad_scan_compact_workspace_bytes": [list(s) for s in SIDES],
    "cmdiad_ccl_workspace_bytes": [[n, h, w] for n in IMAGES for h, w in SIDES[:11] + [(4096, 4096), (4097, 4096), (1 << 13, 1 << 12)]],
    "cmdiad_sort_u64_workspace_bytes": [[n] for n in (-1, 0, 1, 255, 256, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, SORT_TILE + 7, 2 * SORT_TILE,
                                                      2 * SORT_TILE + 1, 32 * 224 * 224, 1 << 30, (1 << 30) + 1)],
    "cmdiad_region_table_workspace_bytes": [[n, h, w] for n in IMAGES for h, w in SIDES[:11] + [(4096, 4096), (4097, 4096), (1 << 13, 1 << 12)]],
}


def main():
    lib = nat.lib()
    queries = {q for q in nat.SIZE_QUERIES if q.endswith("_workspace_bytes")} - {"cmdiad_ocsvm_fit_workspace_bytes"}
    assert queries == set(GRID), queries ^ set(GRID)
    table = {q: [[args, int(getattr(lib, q)(*args))] for args in GRID[q]] for q in sorted(GRID)}
    with open(os.path.join(HERE, "workspace_sizes.json"), "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print({q: len(v) for q, v in table.items()}, sum(len(v) for v in table.values()))


if __name__ == "__main__":
    main()
