"""Vector-instruction count of a kernel's hot loop from `hipcc -S` output.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Imeshdiffusion_amd/csrc --cuda-device-only -S \
        meshdiffusion_amd/csrc/block_pass.hip -o block_pass.s
    python tools/count_isa.py block_pass.s md_block_pass_kernelILi16ELb1 8

Prints, for the function whose mangled name contains the second argument, the instruction mix of the whole function and of its
largest backward-branch loop, the latter also divided by the third argument (the 16-channel steps one trip of that loop holds:
8 for md_block_pass_kernel, whose group-pair loop is not unrolled)."""
import collections
import re
import sys


def classes(lines):
    c = collections.Counter()
    for ins in lines:
        op = ins.split()[0]
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            if "_dpp" in op or " row_" in ins or " wave_" in ins or "quad_perm" in ins:
                c["valu_dpp"] += 1
            for k in ("v_cndmask", "v_med3", "v_cmp_class", "v_max3", "v_max_f32", "v_mul_f32", "v_pk_mul_f32", "v_cvt_f16", "v_cvt_pk",
                      "v_exp", "v_rcp", "v_permlane", "v_mov_b32", "v_cvt_scalef32"):
                if op.startswith(k):
                    c[k] += 1
        elif op.startswith("ds_bpermute"):
            c["ds_bpermute"] += 1
        elif op.startswith("ds_"):
            c["ds_other"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith("s_waitcnt"):
            c["s_waitcnt"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
    return c


def main():
    path, name, steps = sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 1
    body, inside = [], False
    for ln in open(path):
        if not inside:
            if re.match(r"^_Z\w*:", ln) and name in ln:
                inside = True
            continue
        if ln.startswith(".Lfunc_end"):
            break
        body.append(ln.rstrip("\n"))
    assert body, f"no function matching {name}"
    labels, ins = {}, []
    for ln in body:
        s = ln.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            labels[m.group(1)] = len(ins)
        elif not s.startswith("."):
            ins.append(s)
    best = (0, 0)
    for i, s in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", s)
        if m and labels.get(m.group(1), i + 1) <= i and i - labels[m.group(1)] > best[1] - best[0]:
            best = (labels[m.group(1)], i)
    whole, loop = classes(ins), classes(ins[best[0]:best[1] + 1])
    print(f"function: {len(ins)} instructions  " + "  ".join(f"{k} {v}" for k, v in sorted(whole.items())))
    print(f"largest loop: {best[1] + 1 - best[0]} instructions  " + "  ".join(f"{k} {v}" for k, v in sorted(loop.items())))
    if steps > 1:
        print(f"per step (/{steps}): " + "  ".join(f"{k} {v / steps:.1f}" for k, v in sorted(loop.items())))


if __name__ == "__main__":
    main()
