"""The mesh entry points (csrc/mesh.hip: cmdiad_mesh_count, cmdiad_mesh_write; docs/mesh.md) at the size of a predictor batch, 32 x
224 x 224, and of one full-resolution scan, 1 x 800 x 800, on a fully valid and on a half-valid cloud, with both store variants of the
write kernels: records staged in LDS and stored as dwords ('lds'), or every byte a store of its own ('bytes').

The tool loads the test-only build (libcmdiad_hip_ab.so, which carries both variants and follows CMDIAD_MESH_STORE per call) and checks
that the two give the same bytes.  Kernels are timed by HIP events (median of --reps launches after a warm-up) and reported with the
bytes their contract moves at least once (count: the cloud and the maps read; write: those, the float32 background and the labels read,
vidx and the used records written) and the achieved bytes/s.  --class_run adds the `meshes` phase of evaluate.ClassRun beside `predict`
and `overlays` on a small synthetic class; --host adds mesh.save of the batch on the host clock.
Usage: python tools/bench_mesh.py [--reps 20] [--out FILE.md] [--class_run] [--host]"""
import os as _os
_os.environ.setdefault("CMDIAD_HIP_LIB", _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "cmdiad_amd", "libcmdiad_hip_ab.so"))
import argparse  # noqa: E402
import json  # noqa: E402
import os  # noqa: E402
import sys  # noqa: E402
import tempfile  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmdiad_amd import _native as nat  # noqa: E402
from cmdiad_amd import mesh, ops, overlay  # noqa: E402

from bench_overlay import event_ms  # noqa: E402


def synthetic(n, S, valid, dev, seed=0):
    """an organised cloud [n,3,S,S] over a jittered grid with a smooth relief, `valid` of its points kept (the others zero, in
    blobs as a scanner drops them), and maps [n,S,S] f64"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    x = 5.0 + 0.4 * xx[None] + 0.05 * torch.rand((n, S, S), generator=g)
    y = 9.0 + 0.4 * yy[None] + 0.05 * torch.rand((n, S, S), generator=g)
    z = 300.0 + 4.0 * torch.sin(0.05 * x) * torch.cos(0.04 * y) + 0.02 * torch.rand((n, S, S), generator=g)
    cloud = torch.stack([x, y, z], dim=1)
    if valid < 1.0:
        coarse = torch.rand((n, 1, S // 8 + 1, S // 8 + 1), generator=g)
        keep = torch.nn.functional.interpolate(coarse, size=(S, S), mode="bilinear")[:, 0] < torch.quantile(coarse, valid)
        cloud = cloud * keep[:, None]
    maps = torch.rand((n, S, S), generator=g, dtype=torch.float64)
    return cloud.to(dev).contiguous(), maps.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--class_run", action="store_true")
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    if not nat.lib().cmdiad_has_ab_variants():
        raise SystemExit("bench_mesh: the store variants live in the test-only build (make -C cmdiad_amd/csrc ab)")
    dev = torch.device("cuda", torch.cuda.current_device())
    out, lines = dict(kernels={}), ["| entry point | case | store | ms | MB moved at least once | GB/s |", "|---|---|---|---:|---:|---:|"]
    after = [""]          # what goes behind the table

    def row(name, case, store, fn, nbytes):
        ms = event_ms(fn, a.reps)
        out["kernels"][f"{name} {case} {store}"] = dict(ms=round(ms, 4), bytes=int(nbytes), gb_per_s=round(nbytes / ms / 1e6, 1))
        print(f"  {name:18s} {case:28s} {store:6s} {ms:8.3f} ms {nbytes / 1e6:8.1f} MB {nbytes / ms / 1e6:8.1f} GB/s", flush=True)
        lines.append(f"| `{name}` | {case} | {store} | {ms:.3f} | {nbytes / 1e6:.1f} | {nbytes / ms / 1e6:.0f} |")

    for n, S in ((32, 224), (1, 800)):
        spec = overlay.DeviceSpec(mesh.MeshSpec(0.0, 1.0), n, dev)
        bg = torch.randn((n, 3, S, S), device=dev)
        labels = torch.randint(0, 5, (n, S, S), device=dev, dtype=torch.int32)
        for valid in (1.0, 0.5):
            cloud, maps = synthetic(n, S, valid, dev)
            case = f"{n} x {S}^2 {'full' if valid == 1.0 else 'half valid'}"
            got_count = ops.mesh_count(cloud, maps, layout="planar")
            got = ops.mesh_write(cloud, maps, got_count[0], spec.lohi, spec.lut, spec.alpha, background=bg, labels=labels, layout="planar")
            counts = got_count[1].cpu().numpy()
            px = n * S * S
            read = px * 12 + px * 8
            row("cmdiad_mesh_count", case, "-", lambda: ops.mesh_count(cloud, maps, out=got_count, layout="planar"), read)
            written = px * 4 + int(counts[:, 0].sum()) * ops.MESH_VERTEX_BYTES + int(counts[:, 1].sum()) * ops.MESH_FACE_BYTES
            results = {}
            for store in ("bytes", "lds"):
                os.environ["CMDIAD_MESH_STORE"] = store
                for t in got[1:]:
                    t.zero_()
                row("cmdiad_mesh_write", case, store,
                    lambda: ops.mesh_write(cloud, maps, got_count[0], spec.lohi, spec.lut, spec.alpha, background=bg, labels=labels, out=got,
                                           layout="planar"), read + px * 12 + px * 4 + written)
                results[store] = [got[1][i, :counts[i, 0] * ops.MESH_VERTEX_BYTES].clone() for i in range(n)] + \
                                 [got[2][i, :counts[i, 1] * ops.MESH_FACE_BYTES].clone() for i in range(n)]
            os.environ.pop("CMDIAD_MESH_STORE")
            assert all(torch.equal(x, y) for x, y in zip(results["bytes"], results["lds"])), "the store variants differ"
            out.setdefault("counts", {})[case] = dict(vertices=int(counts[:, 0].sum()), faces=int(counts[:, 1].sum()))
            if a.host and n == 32:
                with tempfile.TemporaryDirectory() as tmp:
                    paths = [os.path.join(tmp, f"{i}.ply") for i in range(n)]
                    ms = mesh.MeshSpec(0.0, 1.0)
                    mesh.save(paths, cloud, maps, ms, background=bg, labels=labels, layout="planar")
                    t0 = time.perf_counter()
                    sizes = mesh.save(paths, cloud, maps, ms, background=bg, labels=labels, layout="planar")
                    per_s = n / (time.perf_counter() - t0)
                out.setdefault("host", {})[case] = dict(bytes_per_file=int(np.mean(sizes)), save_files_per_s=round(per_s, 1))
                print(f"  mesh.save {case}: {int(np.mean(sizes))} B/file, {per_s:.1f} files/s", flush=True)
                after.append(f"mesh.save, {case}: {int(np.mean(sizes))} bytes per file, {per_s:.0f} files/s")
    if a.class_run:
        from cmdiad_amd import evaluate as ev
        from cmdiad_amd.models.hallucination_network import HallucinationCrossModalityNetwork
        from cmdiad_amd.models.models import PointTransformer, VisionTransformer
        from cmdiad_amd.synth import SyntheticClass, sharpen_pointmae
        os.environ.setdefault("CMDIAD_ALLOW_RANDOM_INIT", "1")    # synthetic weights, as bench.py's class loop
        torch.manual_seed(0)
        weights = ({k: v.detach() for k, v in VisionTransformer().state_dict().items()},
                   sharpen_pointmae({k: v.detach() for k, v in PointTransformer().state_dict().items()}),
                   {k: v.detach() for k, v in HallucinationCrossModalityNetwork(None, 768, 768).state_dict().items()})
        with tempfile.TemporaryDirectory() as tmp:
            res = ev.run_class(ev.mtfi_args(f_coreset=0.1, random_state=3, calibration_holdout=2, overlay_dir=os.path.join(tmp, "ov"),
                                            mesh_dir=os.path.join(tmp, "mesh")), SyntheticClass("rope", 6, 20, index=8), weights=weights)
        out["class_run"] = {k: res["seconds"].get(k) for k in ("predict", "metrics", "overlays", "meshes")}
        out["class_run"]["files"] = res["meshes"]["files"]
        print(f"  ClassRun (20 test images): {out['class_run']}")
        after += ["", f"ClassRun, synthetic class with 20 test images: predict {res['seconds']['predict']} s, overlays "
                  f"{res['seconds']['overlays']} s, meshes {res['seconds']['meshes']} s ({res['meshes']['files']} files)"]
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines + after) + "\n")


if __name__ == "__main__":
    main()
