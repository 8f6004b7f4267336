"""Generate tests/golden/antialias.npz (build host only, CPU: the GPU machines have no reference):
    python tools/gen_golden_antialias.py [--no-fit]

  case/<mesh>-<H>x<W>/L<layer>/<colour>/ref_err_{value,dcolor,dpos}   per case, layer and colour of tests/antialias_cases.py: the
                      fp32 torch restatement's OWN rel-L2 distance from the float64 one (the `rast` of the restated rasteriser,
                      decisions shared) -- the unit of the GPU tests' bars -- and case/.../active, the number of active pairs.
  alpha/<mesh>-<H>x<W>/ref_err_dverts   the same for d (alpha, alpha_second) / d verts through xfm_points.
  fit/steps, fit/depth32, fit/depth64, fit/alpha32, fit/alpha64   the fitting run of tests/test_gpu_antialias.py (sphere of radius
                      0.9 -> torus, 256 x 256, 4 views, 21 iterations, alpha_weight 1, no chamfer, no carve) with the unmodified
                      reference `DMTetGeometry`, marching tetrahedra and `sdf_reg_loss` and the restated rasteriser, antialiasing
                      and losses on the CPU, in fp32 and in float64: both loss terms at iterations 0, 10, 20.
  fit/iou_small_start   the final silhouette IoU against the target of the float64 loop from a sphere of radius 0.5, which does
                      not cover the target's silhouette, with alpha_weight 0 and 1.
The file holds only such numbers.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import antialias_cases as ac  # noqa: E402
import raster_cases as rc  # noqa: E402
from oracle.gen_golden import GOLD, REF, _CudaToCpu, import_ref_dmtet  # noqa: E402

G_SEED = 9400
C_SEED = 9500
ALPHA_CASES = (ac.CASES[1],)


def gen_cases(out):
    for case in ac.CASES:
        cid = ac.case_id(case)
        pc, faces, H, W = ac.case_inputs(case)
        nbr = torch.as_tensor(ac.edge_neighbours_restated(faces.numpy(), pc.shape[1]))
        for layer, rast in enumerate(ac.rast_restated(pc, faces, H, W)):
            dec = ac.pair_decisions(rast, pc, faces, nbr)
            assert int(dec["n_pass"].max()) <= 1, cid
            for kind in ac.COLOURS:
                col = ac.case_colour(kind, rast[..., 3] > 0, C_SEED)
                G = ac.case_G(col.shape, G_SEED)
                r64 = ac.grads_restated(col, rast, pc, faces, nbr, G, torch.float64, dec)
                r32 = ac.grads_restated(col, rast, pc, faces, nbr, G, torch.float32, dec)
                errs = [rc.rel_l2(a, b) for a, b in zip(r32, r64)]
                key = f"case/{cid}/L{layer}/{kind}"
                for q, e in zip(("value", "dcolor", "dpos"), errs):
                    out[f"{key}/ref_err_{q}"] = np.float64(e)
                print(f"[antialias] {cid} layer {layer} {kind}: active {int(dec['active'].sum())}  fp32 restatement vs float64: "
                      f"value {errs[0]:.2e} d color {errs[1]:.2e} d pos_clip {errs[2]:.2e}")
            out[f"case/{cid}/L{layer}/active"] = np.int64(int(dec["active"].sum()))
    out["case/g_seed"], out["case/c_seed"] = np.int64(G_SEED), np.int64(C_SEED)
    for case in ALPHA_CASES:
        verts, faces = ac.param_torus()
        H, W = case[1:]
        mvp, _ = rc.cameras(rc.ANGLES, H, W)
        rast = ac.rast_restated(rc.xfm_points_restated(verts, mvp), faces, H, W)
        G = ac.case_G((2, mvp.shape[0], H, W, 1), G_SEED)
        g = []
        for dtype in (torch.float32, torch.float64):
            v = verts.detach().clone().to(dtype).requires_grad_(True)
            a1, a2, _, _ = ac.alpha_restated(v, faces, mvp, H, W, dtype, rast)
            ((a1 * G[0]).sum() + (a2 * G[1]).sum()).backward()
            g.append(v.grad)
        out[f"alpha/{ac.case_id(case)}/ref_err_dverts"] = np.float64(rc.rel_l2(g[0], g[1]))
        print(f"[antialias] alpha {ac.case_id(case)}: d verts fp32 restatement vs float64 {rc.rel_l2(g[0], g[1]):.2e}")


def run_fit(mod, dtype, alpha_weight, radius, iters=ac.FIT_ITERS):
    """The loop of meshdiffusion_amd.render.fit_to_views (every view each iteration, no chamfer, no carve) with the reference's
    classes and the restated rasteriser and antialiasing, on the CPU in `dtype`: (depth terms, alpha terms, final IoU)."""
    H = W = ac.FIT_RES
    mvp, campos = rc.cameras(rc.FIT_ANGLES, H, W)
    tv, tf = rc.mesh("torus")
    tgt = rc.targets_restated(tv, tf, mvp, campos, H, W, dtype)
    with torch.no_grad():
        t_alpha, t_alpha2, t_mask, _ = ac.alpha_restated(tv, tf, mvp, H, W, dtype)
    with _CudaToCpu():
        geo = mod.DMTetGeometry(64, 2.1, None, root=os.path.join(REF, "nvdiffrec"), deform_scale=2.0)
        geo.verts = geo.verts.to(dtype)
        with torch.no_grad():
            geo.sdf.data = (geo.verts.norm(dim=1) - radius).clamp(-1.0, 1.0).to(dtype)
            geo.deform.data = torch.zeros_like(geo.verts)
        opt = torch.optim.Adam([geo.sdf, geo.deform], lr=rc.FIT_LR)
        depth_terms, alpha_terms = [], []
        for it in range(iters + 1):                                             # the last pass only measures the silhouette
            if it < iters and it % 300 == 0 and it < 1790:
                geo.deform.data[:] *= 0.4
            opt.zero_grad()
            verts, faces, _, _, _, valid_vert_idx = geo.marching_tets(geo.get_deformed(), geo.sdf, geo.indices)
            pc = rc.xfm_points_restated(verts.detach(), mvp, dtype).to(torch.float32)
            ids = rc.rasterize_restated(pc, faces, H, W)["ids"]
            if it == iters:
                final_iou = ac.iou((ids[:, 0] > 0).to(dtype), t_mask[..., 0])
                break
            d = rc.depth_restated(verts, faces, mvp, campos, ids, dtype)
            loss = rc.depth_loss_restated(d[:, 0, :, :, None], d[:, 1, :, :, None], tgt["depth"], tgt["depth_second"],
                                          tgt["mask_cont"], it)
            a1, a2, _, _ = ac.alpha_restated(verts, faces, mvp, H, W, dtype, ac.rast_restated(pc, faces, H, W, ids))
            alpha = ac.silhouette_loss_restated(a1, a2, t_alpha, t_alpha2)
            sdf_weight = rc.FIT_SDF_REGULARIZER - (rc.FIT_SDF_REGULARIZER - 0.01) * min(1.0, 4.0 * (it / iters))
            sdf_mask = torch.zeros_like(geo.sdf)
            sdf_mask[valid_vert_idx] = 1.0
            sdf_masked = geo.sdf.detach() * sdf_mask + geo.sdf * (1 - sdf_mask)
            reg = mod.sdf_reg_loss(sdf_masked, geo.all_edges).mean() * sdf_weight * 0.1
            total = loss + reg + (alpha * alpha_weight if alpha_weight > 0 else 0.0)
            total.backward()
            opt.step()
            geo.clamp_deform()
            depth_terms.append(float(loss))
            alpha_terms.append(float(alpha))
    return np.array(depth_terms, np.float64), np.array(alpha_terms, np.float64), final_iou


def main():
    if not torch.cuda.is_available():
        torch.Tensor.cuda = lambda self, *a, **k: self      # DMTetGeometry.__init__ hard-codes .cuda()
    out = {}
    gen_cases(out)
    path = os.path.join(GOLD, "antialias.npz")
    if "--no-fit" in sys.argv:                              # keep the fit entries of the file that is there
        old = np.load(path)
        out.update({k: old[k] for k in old.files if k.startswith("fit/")})
    else:
        mod = import_ref_dmtet()
        steps = list(ac.FIT_STEPS)
        d32, a32, _ = run_fit(mod, torch.float32, ac.FIT_ALPHA_WEIGHT, rc.FIT_START_RADIUS)
        d64, a64, iou_big = run_fit(mod, torch.float64, ac.FIT_ALPHA_WEIGHT, rc.FIT_START_RADIUS)
        print("[antialias] fit: depth fp32", d32[steps], "fp64", d64[steps], "alpha fp32", a32[steps], "fp64", a64[steps],
              "final IoU", iou_big)
        ious = [run_fit(mod, torch.float64, w, ac.FIT_SMALL_RADIUS)[2] for w in (0.0, 1.0)]
        print(f"[antialias] fit from radius {ac.FIT_SMALL_RADIUS}: final silhouette IoU with alpha_weight 0 / 1: {ious}")
        out["fit/steps"] = np.array(ac.FIT_STEPS)
        out["fit/depth32"], out["fit/depth64"], out["fit/alpha32"], out["fit/alpha64"] = d32[steps], d64[steps], a32[steps], a64[steps]
        out["fit/iou_small_start"] = np.array(ious, np.float64)
    np.savez_compressed(path, **out)
    print(f"[antialias] wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
