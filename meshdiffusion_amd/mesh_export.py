"""`.npy` sampled grids -> `.obj` meshes, and fitted DMTet dicts -> training grids: the host-side data formats on
either side of the hot path, without nvdiffrast / pytorch3d / pymeshlab.

* `samples_to_obj`: what the tail of the reference's `nvdiffrec/eval.py:385-447` does with the sampler's output
  (`main_diffusion.py --mode=uncond_gen` writes `{eval_dir}/{i}.npy`): gather the tet-grid vertices out of the cubic
  grid, sign / clip, marching tetrahedra (the HIP kernel, 32 meshes per launch), write `{idx:06d}.obj`.  The two other
  steps of that tail are optional keywords, all off by default (the files written are then byte-identical to those without
  them): `preview_dir` renders the reference's quick-look image of each mesh (eval.py:421-438: diffuse, kd = (0.75, 0.3, 0.6),
  an environment light; `render.render_preview`) to `{idx:06d}.png`, and `smooth_steps` / `min_component_*` / `keep_largest`
  run the clean-up of `postprocess.postprocess` (eval.py:449-456) on the whole batch before the `.obj` is written.  Both are
  built in the manner of the reference under the mesh post-processing contract (csrc/meshpost.hip), not bit-equal to
  pymeshlab or nvdiffrast: umbrella smoothing, a floater filter, nine spherical-harmonic coefficients for the environment, and
  with `remesh_iters` > 0 the isotropic remeshing of the remeshing contract (csrc/remesh.hip) before and after the smoothing.
* `save_png` / `load_png`: 8-bit RGB PNG with the standard library's zlib and struct only, quantised with rint(x * 255) as the
  reference's `util.save_image` does.
* `save_obj`: the plain "v x y z" / "f i j k" (1-based) subset of the format `pytorch3d.io.save_obj` writes
  (`eval.py:436-440`).
* `tet_to_grid` / `dicts_to_grids`: `data/tets_to_3dgrid.py:7-49`, the `dmt_dict_{id}.pt` -> `grid_{id}.pt` step that
  produces the training set read by `lib/dataset/shapenet_dmtet_dataset.py`.

    python -m meshdiffusion_amd.mesh_export --sample_path out/0.npy --tet_path 64_tets_cropped.npz --out meshes/
    python -m meshdiffusion_amd.mesh_export --sample_path out/0.npy --tet_path 64_tets_cropped.npz --out meshes/ \\
        --num_smooth_steps 3 --keep_largest --preview_dir previews/
"""
import argparse
import os
import struct
import zlib

import numpy as np
import torch

from .dmtet import GridMesher, tet_vertices_to_grid_index


def save_obj(path, verts, faces, decimal_places=None, normals=None):
    """verts float [V,3], faces int [F,3] (0-based) -> Wavefront OBJ.  normals (optional, float [V,3], one per vertex,
    e.g. dmtet.auto_normals): written as `vn` lines and referenced as `f i//i`."""
    v = torch.as_tensor(verts).detach().cpu().numpy().astype(np.float64)
    f = torch.as_tensor(faces).detach().cpu().numpy().astype(np.int64) + 1
    fmt = "%f" if decimal_places is None else f"%.{int(decimal_places)}f"
    with open(path, "w") as fh:
        for row in v:
            fh.write("v " + " ".join(fmt % c for c in row) + "\n")
        if normals is not None:
            for row in torch.as_tensor(normals).detach().cpu().numpy().astype(np.float64):
                fh.write("vn " + " ".join(fmt % c for c in row) + "\n")
            for row in f:
                fh.write("f %d//%d %d//%d %d//%d\n" % (row[0], row[0], row[1], row[1], row[2], row[2]))
        else:
            for row in f:
                fh.write("f %d %d %d\n" % (row[0], row[1], row[2]))


def load_obj(path):
    """Inverse of save_obj (tests / round trips): returns (verts float32 [V,3], faces int64 [F,3] 0-based)."""
    vs, fs = [], []
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                vs.append([float(c) for c in t[1:4]])
            elif t[0] == "vn":
                continue
            elif t[0] == "f":
                fs.append([int(c.split("/")[0]) - 1 for c in t[1:4]])
    return np.asarray(vs, np.float32).reshape(-1, 3), np.asarray(fs, np.int64).reshape(-1, 3)


_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def save_png(path, img):
    """img [H,W,3], float in [0, 1] (quantised with rint(clip(x, 0, 1) * 255), as the reference's util.save_image) or uint8 -> an
    8-bit RGB PNG, written with zlib and struct only."""
    a = img.detach().cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"save_png: expected an image [H,W,3], got {a.shape}")
    if a.dtype != np.uint8:
        a = np.clip(np.rint(a.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    H, W = a.shape[:2]
    rows = np.concatenate([np.zeros((H, 1), np.uint8), a.reshape(H, W * 3)], 1)          # filter type 0 in front of every row
    with open(path, "wb") as fh:
        fh.write(_PNG_SIGNATURE + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
                 + _png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _png_chunk(b"IEND", b""))


def load_png(path):
    """The inverse of save_png (tests / round trips): an 8-bit RGB, non-interlaced PNG -> uint8 numpy [H,W,3]."""
    data = open(path, "rb").read()
    if data[:8] != _PNG_SIGNATURE:
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, head = 8, [], None
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if zlib.crc32(kind + body) & 0xFFFFFFFF != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            raise ValueError(f"{path}: bad checksum in chunk {kind!r}")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        pos += 12 + n
    if head is None or head[2:] != (8, 2, 0, 0, 0):
        raise ValueError(f"{path}: only 8-bit RGB, non-interlaced PNG files are read")
    W, H = head[:2]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(H, 1 + 3 * W)
    out = np.zeros((H, 3 * W), np.uint8)
    for i in range(H):
        kind, row = int(raw[i, 0]), raw[i, 1:].astype(np.int64)
        up = out[i - 1].astype(np.int64) if i > 0 else np.zeros(3 * W, np.int64)
        if kind == 0:
            rec = row
        elif kind == 2:
            rec = row + up
        elif kind in (1, 3, 4):                                        # Sub, Average, Paeth: each byte needs the one 3 to its left
            rec = np.zeros(3 * W, np.int64)
            for j in range(3 * W):
                a, b, c = (int(rec[j - 3]), int(up[j]), int(up[j - 3])) if j >= 3 else (0, int(up[j]), 0)
                if kind == 1:
                    pred = a
                elif kind == 3:
                    pred = (a + b) // 2
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                rec[j] = (int(row[j]) + pred) & 255
        else:
            raise ValueError(f"{path}: unknown filter type {kind}")
        out[i] = (rec & 255).astype(np.uint8)
    return out.reshape(H, W, 3)


def samples_to_obj(samples, tet_vertices, tet_indices, out_dir, resolution=None, batch=32, device="cuda", start_index=0,
                   with_normals=False, smooth_steps=0, lam=0.5, mu=None, min_component_faces=0, min_component_fraction=0.0,
                   keep_largest=False, preview_dir=None, angle_ind=0, preview_res=512, preview_raw=True, remesh_iters=0,
                   remesh_target_scale=1.0, remesh_project=False):
    """samples: array [M,4,R,R,R] (or a path to the sampler's .npy).  Writes {out_dir}/{i:06d}.obj, returns their paths.
    with_normals: also write the smooth vertex normals the reference computes right after extraction
    (eval.py:422 `mesh.auto_normals`; its own OBJ export, eval.py:436-440, drops them); with a clean-up they are those of the
    cleaned mesh.
    smooth_steps, lam, mu, min_component_faces, min_component_fraction, keep_largest: the clean-up of `postprocess.postprocess`,
    run on each batch of meshes in one set of launches before the files are written (all off by default).
    remesh_iters, remesh_target_scale: `postprocess.remesh` before and after the smoothing, as the reference's tail does (0 = off);
    remesh_project: every remeshing iteration ends by projecting the vertices back onto the surface that remeshing started from.
    preview_dir: also write {preview_dir}/{i:06d}.png, `render.render_preview` at `preview_camera(angle_ind, preview_res)` of the
    raw mesh, as the reference renders before its clean-up, or with preview_raw=False of the cleaned mesh."""
    if isinstance(samples, (str, os.PathLike)):
        samples = np.load(samples)
    samples = np.asarray(samples)
    R = int(resolution or samples.shape[-1])
    mesher = GridMesher(tet_vertices, tet_indices, R, device=device)
    os.makedirs(out_dir, exist_ok=True)
    clean = smooth_steps > 0 or min_component_faces > 0 or min_component_fraction > 0 or keep_largest or remesh_iters > 0
    if preview_dir is not None:
        from .render import preview_camera, render_preview
        os.makedirs(preview_dir, exist_ok=True)
        mvp, campos = preview_camera(angle_ind, preview_res, device=mesher.verts.device)
    paths = []
    for lo in range(0, samples.shape[0], batch):
        meshes = mesher(torch.from_numpy(samples[lo:lo + batch]))
        cleaned = None
        if clean:
            from .postprocess import postprocess
            cleaned = postprocess(meshes, smooth_steps=smooth_steps, lam=lam, mu=mu, min_component_faces=min_component_faces,
                                  min_component_fraction=min_component_fraction, keep_largest=keep_largest, remesh_iters=remesh_iters,
                                  remesh_target_scale=remesh_target_scale, remesh_project=remesh_project)
        for k, (verts, faces, _face_tet) in enumerate(meshes):
            if preview_dir is not None:
                pv, pf = (verts, faces) if preview_raw or cleaned is None else cleaned[k]
                save_png(os.path.join(preview_dir, "{:06d}.png".format(start_index + lo + k)),
                         render_preview(pv, pf, mvp, campos, preview_res)[0])
            if cleaned is not None:
                verts, faces = cleaned[k]
            path = os.path.join(out_dir, "{:06d}.obj".format(start_index + lo + k))
            nrm = None
            if with_normals and verts.shape[0] > 0:
                from .dmtet import auto_normals
                nrm = auto_normals(verts, faces)[0]
            save_obj(path, verts, faces, normals=nrm)
            paths.append(path)
    return paths


def tet_to_grid(grid_index, sdf, deform, resolution):
    """data/tets_to_3dgrid.py:7-15: scatter per-tet-vertex SDF [N] and deformation [N,3] into a [4,R,R,R] grid."""
    idx = torch.as_tensor(grid_index).long()
    grid = torch.zeros(4, resolution, resolution, resolution)
    grid[0, idx[:, 0], idx[:, 1], idx[:, 2]] = torch.as_tensor(sdf, dtype=torch.float32).reshape(-1)
    grid[1:, idx[:, 0], idx[:, 1], idx[:, 2]] = torch.as_tensor(deform, dtype=torch.float32).transpose(0, 1)
    return grid


def dicts_to_grids(tet_vertices, src_dir, dst_dir, resolution, indices):
    """data/tets_to_3dgrid.py:17-49: `{src_dir}/dmt_dict_{i:05d}.pt` ({'sdf', 'deform'}) -> `{dst_dir}/grid_{i:05d}.pt`."""
    idx = tet_vertices_to_grid_index(tet_vertices)
    os.makedirs(dst_dir, exist_ok=True)
    written = []
    for i in indices:
        src = os.path.join(src_dir, "dmt_dict_{:05d}.pt".format(i))
        if not os.path.exists(src):
            continue
        d = torch.load(src, map_location="cpu", weights_only=False)
        dst = os.path.join(dst_dir, "grid_{:05d}.pt".format(i))
        torch.save(tet_to_grid(idx, d["sdf"], d["deform"], resolution), dst)
        written.append(dst)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sample_path", required=True, help=".npy written by --mode=uncond_gen / cond_gen")
    ap.add_argument("--tet_path", required=True, help="<R>_tets_cropped.npz (vertices, indices)")
    ap.add_argument("--out", required=True, help="directory for the .obj files")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--normals", action="store_true", help="write smooth vertex normals (vn) next to the positions")
    ap.add_argument("--num_smooth_steps", type=int, default=0, help="umbrella smoothing steps after extraction (the reference's flag; 0 = off)")
    ap.add_argument("--lam", type=float, default=0.5, help="weight of a smoothing step")
    ap.add_argument("--mu", type=float, default=None, help="weight of the odd steps (Taubin, e.g. -0.53); unset: lam every step")
    ap.add_argument("--min_component_faces", type=int, default=0, help="drop connected components with fewer faces")
    ap.add_argument("--min_component_fraction", type=float, default=0.0, help="drop components below this fraction of the mesh's largest")
    ap.add_argument("--keep_largest", action="store_true", help="keep only the largest connected component of each mesh")
    ap.add_argument("--remesh_iters", type=int, default=0, help="isotropic remeshing iterations before and after the smoothing (0 = off)")
    ap.add_argument("--remesh_target_scale", type=float, default=1.0, help="target edge length as a multiple of each mesh's mean edge length")
    ap.add_argument("--remesh_project", action="store_true", help="end every remeshing iteration by projecting the vertices back onto the input surface")
    ap.add_argument("--preview_dir", default=None, help="directory for a diffuse quick-look PNG of each mesh")
    ap.add_argument("--angle_ind", type=int, default=0, help="camera pose of the preview, 0..50 around the object")
    ap.add_argument("--preview_res", type=int, default=512)
    ap.add_argument("--preview_post", action="store_true", help="render the cleaned mesh instead of the raw one")
    a = ap.parse_args(argv)
    tet = np.load(a.tet_path)
    paths = samples_to_obj(a.sample_path, tet["vertices"], tet["indices"], a.out, batch=a.batch, with_normals=a.normals,
                           smooth_steps=a.num_smooth_steps, lam=a.lam, mu=a.mu, min_component_faces=a.min_component_faces,
                           min_component_fraction=a.min_component_fraction, keep_largest=a.keep_largest, preview_dir=a.preview_dir,
                           angle_ind=a.angle_ind, preview_res=a.preview_res, preview_raw=not a.preview_post, remesh_iters=a.remesh_iters,
                           remesh_target_scale=a.remesh_target_scale, remesh_project=a.remesh_project)
    print(f"wrote {len(paths)} meshes to {a.out}" + (f" and their previews to {a.preview_dir}" if a.preview_dir else ""))


if __name__ == "__main__":
    main()
