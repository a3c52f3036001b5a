"""Static instruction counts of one kernel in a gfx950 assembly listing, split at its s_barriers.

Usage:
  hipcc --offload-arch=gfx950 <the Makefile's CFLAGS> --cuda-device-only -S csrc/group_strip.hip -o gs.s
  python tools/asm_counts.py gs.s [mangled-name substring, default k_group_stripIDF16_Lb0ELb1E]

Per segment (the instructions between two barriers, in listing order -- not execution order:
the listing follows the compiler's block layout) it prints VALU, MFMA, SALU, LDS and vector-memory
counts, then the whole kernel's totals with v_mov_b32 / v_readlane / v_writelane / s_nop / the
conversions broken out, and the kernel's register and scratch figures from its metadata.
An opcode is counted under its base name (the _e32 / _e64 / _sdwa encodings folded in); a _dpp
form is an opcode of its own (v_mov_b32_dpp is not a v_mov_b32); the names ending in "*" below
are families counted by prefix."""
import collections
import re
import sys

def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "k_group_stripIDF16_Lb0ELb1E"
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(want) + r"\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))   # (an early s_endpgm is a return)
    name = lines[start].split(":")[0]


    def kind(op):
        if op.startswith("v_mfma") or op.startswith("v_smfma"):
            return "MFMA"
        if op.startswith("v_"):
            return "VALU"
        if op.startswith("ds_"):
            return "LDS"
        if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
            return "VMEM"
        if op.startswith("s_"):
            return "SALU"
        return "other"


    segs = [collections.Counter()]
    ops = [collections.Counter()]
    for l in lines[start + 1:end + 1]:
        t = l.strip()
        if not t or t.startswith((";", ".", "/")) or t.endswith(":"):
            continue
        op = re.sub(r"_(e32|e64|sdwa)$", "", t.split()[0])
        segs[-1][kind(op)] += 1
        ops[-1][op] += 1
        if op == "s_barrier":
            segs.append(collections.Counter())
            ops.append(collections.Counter())

    WATCH = ("v_mov_b32", "v_mov_b32_dpp", "v_accvgpr*", "v_readlane_b32", "v_writelane_b32", "s_nop", "v_cvt_f32_f16",
             "v_cvt_pk_f16_f32", "v_fma_mix*", "v_pk_fma_f32", "v_pk_add_f32", "v_pk_mul_f32", "v_add_f32", "v_add_f32_dpp",
             "v_add_u32", "v_lshl_add_u32", "v_lshlrev_b32", "v_bitop3*")


    def count(o, w):
        return sum(v for k, v in o.items() if k.startswith(w[:-1])) if w.endswith("*") else o[w]
    print(name)
    print(f"{'seg':>3} {'VALU':>5} {'MFMA':>5} {'SALU':>5} {'LDS':>5} {'VMEM':>5}  notable")
    for i, (s, o) in enumerate(zip(segs, ops)):
        note = ", ".join(f"{count(o, w)} {w}" for w in WATCH if count(o, w) >= 8)
        print(f"{i:>3} {s['VALU']:>5} {s['MFMA']:>5} {s['SALU']:>5} {s['LDS']:>5} {s['VMEM']:>5}  {note}")
    tot, topo = sum(segs, collections.Counter()), sum(ops, collections.Counter())
    print("total", {k: tot[k] for k in ("VALU", "MFMA", "SALU", "LDS", "VMEM")})
    print("of which", {w: count(topo, w) for w in WATCH})
    for l in lines:
        m = re.match(r"\s*\.set " + re.escape(name) + r"\.(num_vgpr|num_agpr|numbered_sgpr|private_seg_size), (\S+)", l)
        if m:
            print(m.group(1), m.group(2))


if __name__ == "__main__":
    main()
