"""Writes tests/golden/texture.npz on the CPU: the bars of tests/test_gpu_texture.py, each the distance of the fp32 restatement of the
texture contract (tests/texture_cases.py) from its float64 restatement, the share of texels the projection cases leave out, and the
round-trip error of the CPU pipeline.  Scalars only.

    python tools/gen_golden_texture.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import texture_cases as tc  # noqa: E402
from meshdiffusion_amd import texture  # noqa: E402


def project_inputs_cpu(case):
    """The buffers of a projection case from the CPU restatements: (bake, views, images, mvp, campos, uvs, uv_idx, verts, faces)."""
    name, n_views, side, R = case
    verts, faces = tc.MESHES[name]()
    uvs, uv_idx = texture.face_atlas(faces.shape[0], R)
    bake = tc.render_uv_cpu(verts, faces, uvs, uv_idx, R)
    mvp, campos = tc.view_cameras(n_views, side)
    views = tc.views_cpu(verts, faces, uvs, uv_idx, mvp, campos, side)
    images = tc.smooth_color(views["pos"]) * views["mask"][..., None]
    return bake, views, images, mvp, campos, uvs, uv_idx, verts, faces


def round_trip_t0(bake):
    """The known texture of the round trip: the smooth colour of the texel's surface point, 0.5 off the surface, one dilation step."""
    t0 = np.where(bake["mask"][..., None] > 0.5, tc.smooth_color(bake["pos"]), 0.5)
    return tc.dilate_restated(t0.astype(np.float32), bake["mask"])[0]


def main():
    out = {}
    for case in tc.BWD_CASES:
        cid = tc.sample_case_id(case)
        tex, uv, rast, G = tc.sample_case_inputs(case)
        boundary = case[5]
        d64, u64, kink = tc.sample_grads_restated(tex, uv, G, rast, boundary, np.float64)
        d32, u32, _ = tc.sample_grads_restated(tex, uv, G, rast, boundary, np.float32)
        out[f"bwd/{cid}/ref_err_dtex"] = tc.rel_l2(d32, d64)
        out[f"bwd/{cid}/ref_err_duv"] = tc.rel_l2(u32[~kink], u64[~kink])
        print(f"bwd {cid}: fp32 restatement vs float64 dtex {out[f'bwd/{cid}/ref_err_dtex']:.2e} duv {out[f'bwd/{cid}/ref_err_duv']:.2e} "
              f"kinks {int(kink.sum())} of {kink.size}")
    for name, (tex, mask) in tc.dilate_cases().items():
        t64, m64, t32, m32, err = tex, mask, tex, mask, 0.0
        for _ in range(3):
            t64, m64 = tc.dilate_restated(t64.astype(np.float32), m64, np.float64)
            t32, m32 = tc.dilate_restated(t32, m32, np.float32)
            assert np.array_equal(m64, m32)
            err = max(err, tc.rel_l2(t32, t64))
        out[f"dilate/{name}/ref_err"] = err
        print(f"dilate {name}: fp32 restatement vs float64 {err:.2e}")
    for case in tc.PROJECT_CASES:
        cid = tc.project_case_id(case)
        bake, views, images, mvp, campos, *_ = project_inputs_cpu(case)
        args = (bake["pos"], bake["normal"], bake["mask"], images, views["depth"], views["mask"], mvp.numpy(), campos.numpy())
        c64, w64, unsafe = tc.project_restated(*args, dtype=np.float64)
        c32, w32, _ = tc.project_restated(*args, dtype=np.float32)
        on = bake["mask"] > 0.5
        keep = on & ~unsafe
        assert np.array_equal(w64[keep] > 0, w32[keep] > 0)
        out[f"project/{cid}/left_out"] = float((unsafe & on).sum() / on.sum())
        out[f"project/{cid}/ref_err_color"] = tc.rel_l2(c32[keep], c64[keep])
        out[f"project/{cid}/ref_err_weight"] = tc.rel_l2(w32[keep], w64[keep])
        print(f"project {cid}: masked {int(on.sum())} seen {int((w64 > 0).sum())} left out {out[f'project/{cid}/left_out']:.4f} fp32 vs "
              f"float64 colour {out[f'project/{cid}/ref_err_color']:.2e} weight {out[f'project/{cid}/ref_err_weight']:.2e}")
        assert out[f"project/{cid}/left_out"] <= tc.MAX_LEFT_OUT
    # the round trip: render T0 from the views (raw kd, no antialiasing), bake it back, compare on the texels a view saw
    bake, views, _, mvp, campos, uvs, uv_idx, verts, faces = project_inputs_cpu(tc.ROUND_TRIP)
    t0 = round_trip_t0(bake)
    images = tc.sample_restated(t0[None].astype(np.float32), views["uv"].astype(np.float32), None, "clamp", np.float64) * views["mask"][..., None]
    t1, w, _ = tc.project_restated(bake["pos"], bake["normal"], bake["mask"], images, views["depth"], views["mask"], mvp.numpy(), campos.numpy())
    seen = w > 0
    err = np.abs(t1 - t0)[seen]
    out["round_trip/cpu_err"] = float(err.max())
    out["round_trip/cpu_mean_err"] = float(err.mean())
    out["round_trip/seen"] = float(seen.sum() / (bake["mask"] > 0.5).sum())
    print(f"round trip {tc.project_case_id(tc.ROUND_TRIP)}: seen {out['round_trip/seen']:.3f} of the masked texels, |T1 - T0| max "
          f"{err.max():.4f} mean {err.mean():.5f}")
    path = os.path.join(ROOT, "tests", "golden", "texture.npz")
    np.savez(path, **{k: np.float64(v) for k, v in out.items()})
    print(f"wrote {path}: {len(out)} scalars, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
