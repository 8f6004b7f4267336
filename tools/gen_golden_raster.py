"""Generate tests/golden/raster.npz (build host only, CPU: the GPU machines have no reference):
    python tools/gen_golden_raster.py

  cam/<helper>/args, cam/<helper>/out   the UNMODIFIED reference's camera helpers (nvdiffrec/lib/render/util.py:193-277, imported
                      with nvdiffrast and imageio stubbed in sys.modules) for a handful of arguments; random_rotation_translation
                      after np.random.seed(cam/rrt/seed).
  case/<mesh>-<H>x<W>/ref_err_{uv,zf,depth,dverts}   per case of tests/raster_cases.py (B = 2 views): the fp32 torch
                      restatement's OWN rel-L2 distance from the float64 one, ids given -- the unit of the GPU tests' bars --
                      and the counts the exclusions are judged by (covered, left out).
  fit/steps, fit/loss32, fit/loss64   the fitting run of tests/test_gpu_raster.py with the unmodified reference `DMTetGeometry`,
                      marching tetrahedra and `sdf_reg_loss` and the restated rasteriser and depth loss on the CPU, in fp32 and
                      in float64: the depth loss at iterations 0, 10, 20, 40.

Asserted before anything is written: the restated camera equals the reference's helpers; per case both exclusions stay under
0.5 % of the covered pixels; the float64 fit falls below half of its first value.  The file holds only such numbers.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import raster_cases as rc  # noqa: E402
from oracle.gen_golden import GOLD, REF, _CudaToCpu, import_ref_dmtet  # noqa: E402

CAM_ARGS = {
    "perspective": [(0.7854, 1.0, 0.1, 1000.0), (float(np.deg2rad(45.0)), 72 / 40, 0.1, 1000.0), (1.1, 0.75, 0.5, 20.0)],
    "translate": [(0.0, 0.0, -3.0), (0.25, -1.5, 2.0)],
    "rotate_x": [(-0.4,), (1.3,)],
    "rotate_y": [(0.7,), (2.1,), (4.71238898038469,)],
}
RRT_SEED, RRT_T = 7, 0.25
G_SEED = 9300


def import_ref_util():
    for name in ("nvdiffrast", "nvdiffrast.torch", "imageio"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location("ref_render_util", os.path.join(REF, "nvdiffrec/lib/render/util.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gen_cameras(out):
    ref = import_ref_util()
    for helper, arg_list in CAM_ARGS.items():
        out[f"cam/{helper}/args"] = np.array(arg_list, np.float64)
        out[f"cam/{helper}/out"] = np.stack([getattr(ref, helper)(*a).numpy() for a in arg_list])
    np.random.seed(RRT_SEED)
    out["cam/rrt/out"] = np.stack([ref.random_rotation_translation(RRT_T).numpy() for _ in range(2)])
    out["cam/rrt/seed"], out["cam/rrt/t"] = np.int64(RRT_SEED), np.float64(RRT_T)
    # the camera of the cases, from the reference's helpers
    for a, (H, W) in ((0.7, (64, 64)), (2.1, (40, 72))):
        mvp = ref.perspective(np.deg2rad(45.0), W / H, 0.1, 1000.0) @ ref.translate(0, 0, -3.0) @ ref.rotate_x(-0.4) @ ref.rotate_y(a)
        assert torch.equal(mvp, rc.camera(a, H, W)[0]), (a, H, W)
    print("[raster] camera helpers recorded; the cases' camera equals the reference's helpers bit for bit")


def gen_cases(out):
    for case in rc.MESH_CASES:
        name, H, W = case
        cid = rc.case_id(case)
        verts, faces = rc.mesh(name)
        mvp, campos = rc.cameras(rc.ANGLES, H, W)
        pc = rc.xfm_points_restated(verts, mvp)
        r = rc.rasterize_restated(pc, faces, H, W)
        order, numeric, covered = rc.check_caps(r, cid)
        ids = r["ids"]
        use = covered & ~order & ~numeric
        u64, v64 = rc.bary_restated(pc, faces, ids)
        u32, v32 = rc.bary_restated(pc, faces, ids, torch.float32)
        z64, z32 = rc.zf_restated(pc, faces, ids), rc.zf_restated(pc, faces, ids, torch.float32)
        assert float((z64 - r["zf"]).abs().max()) < 1e-12, cid
        d64 = rc.depth_restated(verts, faces, mvp, campos, ids)
        d32 = rc.depth_restated(verts, faces, mvp, campos, ids, torch.float32)
        e_uv = rc.rel_l2(torch.stack([u32, v32])[:, use], torch.stack([u64, v64])[:, use])
        e_zf, e_d = rc.rel_l2(z32[use], z64[use]), rc.rel_l2(d32[use], d64[use])
        out[f"case/{cid}/ref_err_uv"], out[f"case/{cid}/ref_err_zf"] = np.float64(e_uv), np.float64(e_zf)
        out[f"case/{cid}/ref_err_depth"] = np.float64(e_d)
        out[f"case/{cid}/covered"] = np.array([int(covered[:, 0].sum()), int(covered[:, 1].sum())], np.int64)
        msg = f"[raster] {cid}: V={verts.shape[0]} F={faces.shape[0]}  fp32 restatement vs float64: uv {e_uv:.2e} zf {e_zf:.2e} depth {e_d:.2e}"
        if case in rc.GRAD_CASES:
            G = rc.case_G(tuple(ids.shape), G_SEED) * use
            g64 = rc.grad_restated(verts, faces, mvp, campos, ids, G)
            g32 = rc.grad_restated(verts, faces, mvp, campos, ids, G, torch.float32)
            e_g = rc.rel_l2(g32, g64)
            out[f"case/{cid}/ref_err_dverts"] = np.float64(e_g)
            msg += f" d verts {e_g:.2e}"
        assert all(0 < float(out[f"case/{cid}/ref_err_{k}"]) < 1e-4 for k in ("uv", "zf", "depth")), cid
        print(msg)
    out["case/g_seed"] = np.int64(G_SEED)


def run_fit(mod, dtype, lr=None, iters=None):
    """The loop of meshdiffusion_amd.render.fit_to_views (every view each iteration, no chamfer, no carve) with the reference's
    classes and the restated rasteriser, on the CPU in `dtype`."""
    lr = rc.FIT_LR if lr is None else lr
    iters = rc.FIT_ITERS if iters is None else iters
    mvp, campos = rc.fit_cameras()
    tv, tf = rc.mesh("torus")
    H = W = rc.FIT_RES
    tgt = rc.targets_restated(tv, tf, mvp, campos, H, W, dtype)
    with _CudaToCpu():
        geo = mod.DMTetGeometry(64, 2.1, None, root=os.path.join(REF, "nvdiffrec"), deform_scale=2.0)
        geo.verts = geo.verts.to(dtype)
        with torch.no_grad():
            geo.sdf.data = rc.fit_initial_sdf(geo.verts).to(dtype)
            geo.deform.data = torch.zeros_like(geo.verts)
        opt = torch.optim.Adam([geo.sdf, geo.deform], lr=lr)
        losses = []
        for it in range(iters):
            if it % 300 == 0 and it < 1790:
                geo.deform.data[:] *= 0.4
            opt.zero_grad()
            verts, faces, _, _, _, valid_vert_idx = geo.marching_tets(geo.get_deformed(), geo.sdf, geo.indices)
            pc = rc.xfm_points_restated(verts.detach(), mvp, dtype).to(torch.float32)
            ids = rc.rasterize_restated(pc, faces, H, W)["ids"]
            d = rc.depth_restated(verts, faces, mvp, campos, ids, dtype)
            loss = rc.depth_loss_restated(d[:, 0, :, :, None], d[:, 1, :, :, None], tgt["depth"], tgt["depth_second"],
                                          tgt["mask_cont"], it)
            sdf_weight = rc.FIT_SDF_REGULARIZER - (rc.FIT_SDF_REGULARIZER - 0.01) * min(1.0, 4.0 * (it / iters))
            sdf_mask = torch.zeros_like(geo.sdf)
            sdf_mask[valid_vert_idx] = 1.0
            sdf_masked = geo.sdf.detach() * sdf_mask + geo.sdf * (1 - sdf_mask)
            reg = mod.sdf_reg_loss(sdf_masked, geo.all_edges).mean() * sdf_weight * 0.1
            (loss + reg).backward()
            opt.step()
            geo.clamp_deform()
            losses.append(float(loss))
    return np.array(losses, np.float64)


def main():
    if not torch.cuda.is_available():
        torch.Tensor.cuda = lambda self, *a, **k: self      # DMTetGeometry.__init__ hard-codes .cuda()
    out = {}
    gen_cameras(out)
    gen_cases(out)
    mod = import_ref_dmtet()
    if "--scan" in sys.argv:                                # hyper-parameter scan of the float64 loop (prints only)
        for lr in (0.01, 0.03, 0.1):
            l = run_fit(mod, torch.float64, lr=lr)
            print(f"[raster] scan lr {lr}: {l[list(rc.FIT_STEPS)]}")
        return
    l32, l64 = run_fit(mod, torch.float32)[list(rc.FIT_STEPS)], run_fit(mod, torch.float64)[list(rc.FIT_STEPS)]
    print("[raster] fit: depth loss fp32", l32, " fp64", l64, " rel gap", np.abs(l32 - l64) / l64)
    assert l64[-1] < 0.5 * l64[0], "the float64 fitting run must fall below half of its first value: fix its hyper-parameters"
    out["fit/steps"], out["fit/loss32"], out["fit/loss64"] = np.array(rc.FIT_STEPS), l32, l64
    path = os.path.join(GOLD, "raster.npz")
    np.savez_compressed(path, **out)
    print(f"[raster] wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
