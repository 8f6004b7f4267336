"""Generate tests/golden/pointcloud.npz (build host only: the GPU machines have no reference):
    python tools/gen_golden_pointcloud.py

  sample/<case>/...   the UNMODIFIED reference `sample_points(vertices, faces, S, areas=...)` of
                      nvdiffrec/lib/geometry/utils.py on the meshes of tests/pointcloud_cases.py (`areas` is passed because
                      the reference's `_base_face_areas` is undefined).  `torch.rand` is wrapped during the call, so the file
                      holds the reference's face_choices (drawn by `multinomial`), its raw uniforms r_u, r_v and its points.
  sample/<case>/ref_err_grad   the fp32 torch restatement's OWN rel-L2 distance from the float64 restatement of d verts:
                      the unit of the GPU test's bar.
  chamfer/<case>/ref_err_{value,dp1,dp2}   the same for the chamfer value and both gradients (neighbours from float64).
  fit/...             the fitting run of tests/test_gpu_pointcloud.py on the CPU with the unmodified reference `DMTet`,
                      `sdf_reg_loss` and `DMTetGeometry`, the reference's interpolation (`_base_sample_points_selected_faces`
                      fed the explicit uniforms through the wrapped `torch.rand`) and the restated inverse CDF and chamfer,
                      in fp32 and in float64: the chamfer value at iterations 0, 10, 20, 40 of both.

Before anything is written the float64 sampling restatement is asserted against the reference's points, and the float64
fitting run is asserted to fall below half of its first value.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pointcloud_cases as pc  # noqa: E402
from oracle.gen_golden import GOLD, REF, _CudaToCpu, import_ref_dmtet  # noqa: E402


def import_ref_utils():
    spec = importlib.util.spec_from_file_location("ref_geometry_utils", os.path.join(REF, "nvdiffrec/lib/geometry/utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class RandTap:
    """Wraps torch.rand: records every draw, or -- with `feed` -- returns the given tensors instead of drawing."""

    def __init__(self, feed=None):
        self.feed, self.seen = list(feed) if feed is not None else None, []

    def __enter__(self):
        self._orig = torch.rand

        def rand(*a, **k):
            if self.feed is not None:
                ref = self._orig(*a, **k)
                out = self.feed.pop(0).reshape(ref.shape).to(ref.dtype)
            else:
                out = self._orig(*a, **k)
            self.seen.append(out)
            return out
        torch.rand = rand
        return self

    def __exit__(self, *exc):
        torch.rand = self._orig


def gen_sampling(ref, out):
    for name in pc.SAMPLE_CASES:
        verts, faces = pc.sample_case(name)
        B, S = verts.shape[0], pc.SAMPLE_SIZES[name]
        areas = pc.face_areas_restated(verts, faces, torch.float32)
        torch.manual_seed(pc.SAMPLE_SEEDS[name])
        with RandTap() as tap:
            points, choices = ref.sample_points(verts, faces, S, areas=areas)
        assert len(tap.seen) == 2 and points.shape == (B, S, 3) and choices.shape == (B, S) and choices.dtype == torch.int64
        r_u, r_v = tap.seen[0][..., 0], tap.seen[1][..., 0]
        assert bool((areas.gather(1, choices) > 0).all()), name
        p64, _ = pc.sample_points_restated(verts, faces, choices, r_u, r_v)
        err = float((p64 - points.double()).abs().max())
        bound = 4 * 2.0 ** -24 * float(verts.abs().max())
        assert err <= bound, (name, err, bound)
        G = pc.case_G((B, S, 3), pc.SAMPLE_SEEDS[name] + 50)
        g64 = pc.sample_points_grad_restated(verts, faces, choices, r_u, r_v, G)
        g32 = pc.sample_points_grad_restated(verts, faces, choices, r_u, r_v, G, torch.float32)
        eg = pc.rel_l2(g32, g64)
        print(f"[pointcloud] sample {name}: B={B} V={verts.shape[1]} F={faces.shape[0]} S={S}  restatement vs reference "
              f"max|d| {err:.2e} (bound {bound:.2e})  fp32 restatement d verts vs float64 {eg:.2e}")
        out[f"sample/{name}/choices"] = choices.numpy().astype(np.int32)
        out[f"sample/{name}/r_u"], out[f"sample/{name}/r_v"] = r_u.numpy(), r_v.numpy()
        out[f"sample/{name}/points"] = points.numpy()
        out[f"sample/{name}/ref_err_grad"] = np.float64(eg)


def gen_chamfer(out):
    for name in pc.CHAMFER_CASES:
        p, q, w1, w2 = pc.chamfer_case(name)
        _, i12, _ = pc.nn_float64(p, q)
        _, i21, _ = pc.nn_float64(q, p)
        g = pc.chamfer_cotangent(p.shape[0])
        v64, a64, b64 = pc.chamfer_restated(p, q, w1, w2, i12, i21, torch.float64, g)
        v32, a32, b32 = pc.chamfer_restated(p, q, w1, w2, i12, i21, torch.float32, g)
        ev, ea, eb = pc.rel_l2(v32, v64), pc.rel_l2(a32, a64), pc.rel_l2(b32, b64)
        print(f"[pointcloud] chamfer {name}: value {v64.tolist()}  fp32 restatement vs float64: value {ev:.2e} dp1 {ea:.2e} dp2 {eb:.2e}")
        assert 0 < ev < 1e-6 and 0 < ea < 1e-6 and 0 < eb < 1e-6, name
        out[f"chamfer/{name}/value64"] = v64.numpy()
        out[f"chamfer/{name}/ref_err_value"], out[f"chamfer/{name}/ref_err_dp1"] = np.float64(ev), np.float64(ea)
        out[f"chamfer/{name}/ref_err_dp2"] = np.float64(eb)


def _kd_nn(a, b):
    """Index of the nearest point of b for every point of a (float64 k-d tree on the detached values)."""
    return torch.as_tensor(cKDTree(b.detach().double().numpy()).query(a.detach().double().numpy())[1], dtype=torch.int64)


def run_fit(mod, ref, dtype):
    """The loop of meshdiffusion_amd.pointcloud.fit_to_points with the reference's classes, on the CPU in `dtype`."""
    target = pc.fit_target().to(dtype)
    with _CudaToCpu():
        geo = mod.DMTetGeometry(64, 2.1, None, root=os.path.join(REF, "nvdiffrec"), deform_scale=2.0)
        geo.verts = geo.verts.to(dtype)
        with torch.no_grad():
            geo.sdf.data = pc.fit_initial_sdf(geo.verts).to(dtype)
            geo.deform.data = torch.zeros_like(geo.verts)
        opt = torch.optim.Adam([geo.sdf, geo.deform], lr=pc.FIT_LR)
        losses = []
        for it in range(pc.FIT_ITERS):
            opt.zero_grad()
            verts, faces, _, _, _, valid_vert_idx = geo.marching_tets(geo.get_deformed(), geo.sdf, geo.indices)
            r_face, r_u, r_v = pc.fit_uniforms(it)
            areas = pc.face_areas_restated(verts.detach()[None], faces, dtype)
            choices, _ = pc.face_choices_restated(areas, r_face)
            tri = faces[choices[0]]
            with RandTap(feed=[r_u, r_v]):
                pred, _ = ref._base_sample_points_selected_faces(tuple(verts[tri[:, k]][None] for k in range(3)))
            pred = pred[0]
            i12, i21 = _kd_nn(pred, target), _kd_nn(target, pred)
            chamfer = ((pred - target[i12]) ** 2).sum(-1).mean() + ((target - pred[i21]) ** 2).sum(-1).mean()
            sdf_weight = pc.FIT_SDF_REGULARIZER - (pc.FIT_SDF_REGULARIZER - 0.01) * min(1.0, 4.0 * (it / pc.FIT_ITERS))
            sdf_mask = torch.zeros_like(geo.sdf)
            sdf_mask[valid_vert_idx] = 1.0
            sdf_masked = geo.sdf.detach() * sdf_mask + geo.sdf * (1 - sdf_mask)
            reg = mod.sdf_reg_loss(sdf_masked, geo.all_edges).mean() * sdf_weight * 0.1
            (chamfer + reg).backward()
            opt.step()
            geo.clamp_deform()
            losses.append(float(chamfer))
    return np.array([losses[k] for k in pc.FIT_STEPS], np.float64)


def main():
    if not torch.cuda.is_available():
        torch.Tensor.cuda = lambda self, *a, **k: self      # DMTetGeometry.__init__ hard-codes .cuda()
    ref = import_ref_utils()
    out = {}
    gen_sampling(ref, out)
    gen_chamfer(out)
    mod = import_ref_dmtet()
    l32, l64 = run_fit(mod, ref, torch.float32), run_fit(mod, ref, torch.float64)
    print("[pointcloud] fit: chamfer fp32", l32, " fp64", l64, " rel gap", np.abs(l32 - l64) / l64)
    assert l64[-1] < 0.5 * l64[0], "the float64 fitting run must fall below half of its first value: fix its hyper-parameters"
    out["fit/steps"], out["fit/loss32"], out["fit/loss64"] = np.array(pc.FIT_STEPS), l32, l64
    path = os.path.join(GOLD, "pointcloud.npz")
    np.savez_compressed(path, **out)
    print(f"[pointcloud] wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
