"""MMD / COV / 1-NNA (chamfer distance; with --emd the earth mover's distance, with --lfd a light-field distance too) and JSD of generated shapes against a reference set.

    python tools/eval_shapes.py --samples meshes/ --ref reference_meshes/ [--points 2048] [--normalize bbox] [--out metrics.json]
    python tools/eval_shapes.py --samples meshes/ --ref reference_meshes/ --emd --jsd
    python tools/eval_shapes.py --samples out/0.npy --tet_path 64_tets_cropped.npz --ref reference_meshes/
    python tools/eval_shapes.py --samples meshes/ --ref reference_meshes/ --lfd [--lfd_res 256] [--lfd_fields 10]

--samples and --ref are directories of `.obj` files (read in sorted order), or --samples the sampler's `.npy` of grids, which
goes through marching tetrahedra (`GridMesher`, needs --tet_path).  Every mesh is sampled at --points surface points
(`meshdiffusion_amd.metrics.clouds_from_meshes`; one device generator seeded with --seed draws for the samples, then for the
references), normalised (`normalize_clouds`) and handed to `shape_metrics`.  Meshes without faces are left out and counted.
--emd adds MMD / COV / 1-NNA under the earth mover's distance (`emd_matrix`, at most 2048 points), --jsd the Jensen-Shannon
divergence of the two sets' occupancy of a 28^3 grid over [-0.5, 0.5]^3, which is where --normalize bbox puts the clouds.
--lfd adds MMD / COV / 1-NNA under the light-field distance of `meshdiffusion_amd.lfd` (the MESHES, not the sampled clouds: --lfd_fields
light fields of 10 silhouettes at --lfd_res pixels each, through the rasteriser): "mmd_lfd", "cov_lfd", "1nna_lfd", "1nna_lfd_sample",
"1nna_lfd_ref", "lfd_res", "lfd_fields", "skipped_sample_lfd", "skipped_ref_lfd".  It is LFD in the manner of Chen et al. 2003, not
their executable (no contour tracing, other scalings): the values compare with each other, not with numbers from that executable.
Prints one JSON line: the figures of `shape_metrics`, `skipped_sample`, `skipped_ref` and wall `seconds`.  GPU only."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_meshes(path, tet_path=None, batch=32):
    """A directory of .obj files, or a .npy of grids [M,4,R,R,R] -> list of (verts, faces)."""
    from meshdiffusion_amd import mesh_export
    if os.path.isdir(path):
        names = sorted(n for n in os.listdir(path) if n.lower().endswith(".obj"))
        if not names:
            raise SystemExit(f"eval_shapes.py: no .obj files in {path}")
        return [mesh_export.load_obj(os.path.join(path, n)) for n in names]
    if not path.endswith(".npy"):
        raise SystemExit(f"eval_shapes.py: {path} is neither a directory of .obj files nor a .npy of grids")
    if tet_path is None:
        raise SystemExit("eval_shapes.py: a .npy of grids needs --tet_path")
    from meshdiffusion_amd.dmtet import GridMesher
    grids, tet = np.load(path), np.load(tet_path)
    mesher = GridMesher(tet["vertices"], tet["indices"], grids.shape[-1])
    meshes = []
    for lo in range(0, grids.shape[0], batch):
        meshes += [(v.detach(), f) for v, f, _face_tet in mesher(torch.from_numpy(grids[lo:lo + batch]))]
    return meshes


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", required=True, help="directory of .obj files, or the sampler's .npy of grids")
    ap.add_argument("--tet_path", default=None, help="<R>_tets_cropped.npz (vertices, indices), for a .npy of grids")
    ap.add_argument("--ref", required=True, help="directory of reference .obj files")
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--normalize", choices=("bbox", "none"), default="bbox")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--emd", action="store_true", help="also MMD / COV / 1-NNA under the earth mover's distance")
    ap.add_argument("--jsd", action="store_true", help="also the Jensen-Shannon divergence of the occupancy grids")
    ap.add_argument("--lfd", action="store_true", help="also MMD / COV / 1-NNA under the light-field distance of the meshes")
    ap.add_argument("--lfd_res", type=int, default=256, help="silhouette resolution of --lfd (at most 512)")
    ap.add_argument("--lfd_fields", type=int, default=10, help="light fields per mesh of --lfd (at most 16)")
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_shapes.py needs a GPU: the HIP path has no CPU fallback")
    from meshdiffusion_amd.metrics import clouds_from_meshes, normalize_clouds, shape_metrics

    t0 = time.time()
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    sample_meshes, ref_meshes = load_meshes(a.samples, a.tet_path), load_meshes(a.ref)
    s, skipped_s = clouds_from_meshes(sample_meshes, a.points, generator=gen, skip_empty=True)
    r, skipped_r = clouds_from_meshes(ref_meshes, a.points, generator=gen, skip_empty=True)
    extra = {k: True for k in ("emd", "jsd") if getattr(a, k)}                 # without them: the call and the record of before
    rec = shape_metrics(normalize_clouds(s, a.normalize), normalize_clouds(r, a.normalize), **extra)
    if a.lfd:
        from meshdiffusion_amd.lfd import lfd_descriptors, lfd_metrics
        ds, lfd_skipped_s = lfd_descriptors(sample_meshes, a.lfd_res, a.lfd_fields, skip_empty=True)
        dr, lfd_skipped_r = lfd_descriptors(ref_meshes, a.lfd_res, a.lfd_fields, skip_empty=True)
        m = lfd_metrics(ds, dr)
        rec.update({k: m[k] for k in ("mmd_lfd", "cov_lfd", "1nna_lfd", "1nna_lfd_sample", "1nna_lfd_ref")})
        rec.update(lfd_res=a.lfd_res, lfd_fields=a.lfd_fields, skipped_sample_lfd=len(lfd_skipped_s), skipped_ref_lfd=len(lfd_skipped_r))
    torch.cuda.synchronize()
    rec.update(skipped_sample=len(skipped_s), skipped_ref=len(skipped_r), seconds=round(time.time() - t0, 3))
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f)


if __name__ == "__main__":
    main()
