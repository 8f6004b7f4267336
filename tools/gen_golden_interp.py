"""Generate tests/golden/interp.npz (build host only, CPU, seeded):
    python tools/gen_golden_interp.py

  case/<mesh>-<H>x<W>/L<layer>/<tri>/C<C>/Ba<1|B>/ref_err_{value,dattr,drast}   per case, layer and attribute case of
                      tests/interp_cases.py: the fp32 torch restatement's OWN rel-L2 distance from the float64 one (the `rast` of
                      the restated rasteriser) -- the unit of the GPU tests' bars.
  case/<mesh>-<H>x<W>/L<layer>/ref_err_{dpos,depth}   the same for the barycentric backward and for |interpolate(verts) - campos|.
  case/<mesh>-<H>x<W>/ref_err_chain_dverts            ... for d verts of both depth layers through both paths.
  normals/<mesh>/ref_err_{value,dverts}               ... for the vertex normals.
  buffers/<mesh>-<H>x<W>/ref_err_dverts, .../kink, .../min_geo_view   ... for d verts of a seeded G over normal, pos, shaded of both
                      layers; the number of kink pixels and the smallest |geo . view| of a covered pixel per layer.
  fit/steps, fit/{depth,alpha,color}{32,64}           the fitting run of tests/test_gpu_interp.py (sphere of radius 0.9 -> torus,
                      64 x 64, 4 views, 21 iterations, colour and alpha weight 1, no chamfer, no carve) with the unmodified
                      reference `DMTetGeometry`, marching tetrahedra and `sdf_reg_loss` and the restated renderer, in fp32 and
                      float64: the three terms at iterations 0, 10, 20.
Two conditions are asserted: no covered pixel of a buffer case or of the fit's target has |geo . view| < 1e-3 in float64, and the
kink pixels of a case and layer number at most rc.EXCLUDE_CAP of its covered pixels.  The file holds only such numbers and seeds.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import antialias_cases as ac  # noqa: E402
import interp_cases as ic  # noqa: E402
import raster_cases as rc  # noqa: E402

GOLD = rc.GOLD
A_SEED, G_SEED = 9600, 9700


def check_conditions(buf, name):
    """The two conditions of the docstring for the float64 buffers of one case; returns (kink counts, smallest |geo . view|)."""
    kinks, mins = [], []
    for tail in ("", "_second"):
        cov = buf["mask" + tail][..., 0] > 0
        n = int(cov.sum())
        gv = float(buf["geo_view" + tail][cov].abs().min()) if n else float("inf")
        k = int(buf["kink" + tail].sum())
        print(f"[interp] {name} layer{tail or '_first'}: covered {n} smallest |geo . view| {gv:.2e} kink pixels {k}")
        assert gv >= ic.FLIP_MARGIN, (name, tail, gv)
        assert k <= rc.EXCLUDE_CAP * n, (name, tail, k, n)
        kinks.append(k)
        mins.append(gv)
    return kinks, mins


def gen_cases(out):
    for case in ic.CASES:
        cid = ic.case_id(case)
        verts, faces, mvp, campos, pc, H, W = ic.case_inputs(case)
        rast = ac.rast_restated(pc, faces, H, W)
        B, V, F = pc.shape[0], verts.shape[0], faces.shape[0]
        for layer, r in enumerate(rast):
            for name, tri, N, C, Ba in ic.attr_cases(V, F, faces, B):
                attr = ic.case_attr(N, C, Ba, A_SEED)
                G = ic.case_G((B, H, W, C), G_SEED)
                r64 = ic.interpolate_grads_restated(attr, r, tri, G, torch.float64)
                r32 = ic.interpolate_grads_restated(attr, r, tri, G, torch.float32)
                for q, a, b in zip(("value", "dattr", "drast"), r32, r64):
                    out[f"case/{cid}/L{layer}/{name}/ref_err_{q}"] = np.float64(rc.rel_l2(a, b) if float(b.abs().max()) > 0 else 0.0)
            G4 = ic.case_G((B, H, W, 4), G_SEED + 1)
            e = rc.rel_l2(ic.bary_grad_restated(pc, faces, r, G4, torch.float32), ic.bary_grad_restated(pc, faces, r, G4, torch.float64))
            out[f"case/{cid}/L{layer}/ref_err_dpos"] = np.float64(e)
            d32, d64 = (ic.chain_depth_restated(verts, faces, mvp, campos, r, t) for t in (torch.float32, torch.float64))
            out[f"case/{cid}/L{layer}/ref_err_depth"] = np.float64(rc.rel_l2(d32, d64))
            print(f"[interp] {cid} layer {layer}: covered {int(ic.covered(r, F).sum())}  fp32 restatement vs float64: d pos_clip {e:.2e} "
                  f"depth {rc.rel_l2(d32, d64):.2e} value/dattr/drast (faces, C3, Ba1) "
                  + " ".join(f"{float(out[f'case/{cid}/L{layer}/faces/C3/Ba1/ref_err_{q}']):.2e}" for q in ("value", "dattr", "drast")))
        ids = torch.stack([rast[0][..., 3], rast[1][..., 3]], 1).to(torch.int64)
        Gd = ic.case_G((B, 2, H, W), G_SEED + 2)
        g32, g64 = (rc.grad_restated(verts, faces, mvp, campos, ids, Gd, t) for t in (torch.float32, torch.float64))
        out[f"case/{cid}/ref_err_chain_dverts"] = np.float64(rc.rel_l2(g32, g64))
    for name in sorted({c[0] for c in ic.CASES}):
        verts, faces = ic.mesh(name)
        G = ic.case_G(verts.shape, G_SEED + 3)
        n32, g32 = ic.vertex_normals_grads_restated(verts, faces, G, torch.float32)
        n64, g64 = ic.vertex_normals_grads_restated(verts, faces, G, torch.float64)
        out[f"normals/{name}/ref_err_value"], out[f"normals/{name}/ref_err_dverts"] = np.float64(rc.rel_l2(n32, n64)), np.float64(rc.rel_l2(g32, g64))
        print(f"[interp] normals {name}: fp32 restatement vs float64 value {rc.rel_l2(n32, n64):.2e} d verts {rc.rel_l2(g32, g64):.2e}")
    for case in ic.BUFFER_CASES:
        cid = ic.case_id(case)
        verts, faces, mvp, campos, pc, H, W = ic.case_inputs(case)
        rast = ac.rast_restated(pc, faces, H, W)
        nbr = torch.as_tensor(ac.edge_neighbours_restated(faces.numpy(), verts.shape[0]))
        dec = [ac.pair_decisions(r, pc, faces, nbr) for r in rast]
        with torch.no_grad():
            buf = ic.buffers_restated(verts, faces, mvp, campos, rast, torch.float64, dec=dec)
        kinks, mins = check_conditions(buf, cid)
        G = ic.buffer_G(buf, G_SEED + 10)
        g32, g64 = (ic.buffers_dverts_restated(verts, faces, mvp, campos, rast, G, t, dec) for t in (torch.float32, torch.float64))
        out[f"buffers/{cid}/ref_err_dverts"] = np.float64(rc.rel_l2(g32, g64))
        out[f"buffers/{cid}/kink"], out[f"buffers/{cid}/min_geo_view"] = np.array(kinks, np.int64), np.array(mins, np.float64)
        print(f"[interp] buffers {cid}: d verts fp32 restatement vs float64 {rc.rel_l2(g32, g64):.2e}")
    out["case/a_seed"], out["case/g_seed"] = np.int64(A_SEED), np.int64(G_SEED)


def run_fit(mod, dtype):
    from oracle.gen_golden import REF, _CudaToCpu
    with _CudaToCpu():
        geo = mod.DMTetGeometry(64, rc.MESH_SCALE, None, root=os.path.join(REF, "nvdiffrec"), deform_scale=2.0)
        geo.verts = geo.verts.to(dtype)
        with torch.no_grad():
            geo.sdf.data = (geo.verts.norm(dim=1) - rc.FIT_START_RADIUS).clamp(-1.0, 1.0).to(dtype)
            geo.deform.data = torch.zeros_like(geo.verts)
        return ic.fit_restated(geo, mod.sdf_reg_loss, dtype)


def main():
    if not torch.cuda.is_available():
        torch.Tensor.cuda = lambda self, *a, **k: self      # DMTetGeometry.__init__ hard-codes .cuda()
    out = {}
    gen_cases(out)
    path = os.path.join(GOLD, "interp.npz")
    from oracle.gen_golden import import_ref_dmtet
    mod = import_ref_dmtet()
    H = W = ic.FIT_RES
    mvp, campos = rc.cameras(rc.FIT_ANGLES, H, W)
    tv, tf = rc.mesh("torus")
    with torch.no_grad():
        tb = ic.buffers_restated(tv, tf, mvp, campos, ac.rast_restated(rc.xfm_points_restated(tv, mvp), tf, H, W), torch.float64)
    check_conditions(tb, "fit target")
    steps = list(ic.FIT_STEPS)
    t32, t64 = run_fit(mod, torch.float32), run_fit(mod, torch.float64)
    out["fit/steps"] = np.array(ic.FIT_STEPS)
    for k in ("depth", "alpha", "color"):
        out[f"fit/{k}32"], out[f"fit/{k}64"] = np.array(t32[k], np.float64)[steps], np.array(t64[k], np.float64)[steps]
        print(f"[interp] fit: {k} fp32 {out[f'fit/{k}32']} float64 {out[f'fit/{k}64']}")
    np.savez_compressed(path, **out)
    print(f"[interp] wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
