#!/usr/bin/env python3
"""
Static instruction counts of the evaluation step's kernels from a device listing of csrc/plan.hip:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Iinclude -Ibluest_amd/csrc bluest_amd/csrc/plan.hip -o plan.s
    python tools/isa_counts.py plan.s

Per Phi kernel: all instructions of the listing (every block once -- which is what a wavefront executes when iters = 1 and
n_cand = 1, minus the block a branch skips), split into VALU / SALU / VMEM / SMEM, the instructions in front of the first
streaming load, those behind the loop's last FMA (the tail), the waits in front of the stream, and the registers.
For k_solve_grad<20,5>: the line numbers (relative to the kernel's start) of the descriptor load, the late kernarg loads, the
first load of the fold, the barriers and the first non-temporal tile load, with the waits between the first barrier and that load.
"""
import re
import sys

PHI = [("k_phi_chunks_shared<%d,1,uint16_t>" % ob, "_Z19k_phi_chunks_sharedILi%dELi1EtE" % ob) for ob in (2, 4, 8)]
PHI.append(("k_phi_chunks<1,uint16_t>", "_Z12k_phi_chunksILi1EtE"))
SOLVE = ("k_solve_grad<20,5>", "_Z12k_solve_gradILi20ELi5EE")


def kernel_body(lines, prefix):
    start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and l.split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    meta = {}
    for l in lines[end:end + 120]:
        m = re.match(r"\s*;\s*(NumVgprs|NumSgprs|Occupancy|ScratchSize|NumAgprs):\s*(\d+)", l)
        if m:
            meta[m.group(1)] = int(m.group(2))
    return start, [l for l in lines[start + 1:end + 1]], meta


def instrs(body):
    out = []
    for l in body:
        t = l.strip()
        if not t or t.startswith((";", ".", "//")) or t.endswith(":") or re.match(r"^[.\w$]+:", t):
            continue
        out.append(t.split(";")[0].strip())
    return out


def kind(ins):
    op = ins.split()[0]
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    if op.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("v_"):
        return "VALU"
    return "SALU"


def phi_report(name, body, meta):
    ins = instrs(body)
    n = {k: 0 for k in ("VALU", "SALU", "VMEM", "SMEM", "LDS")}
    for i in ins:
        n[kind(i)] += 1
    stream = [i for i, x in enumerate(ins) if re.match(r"global_load_dwordx(2|4)", x)]
    first = stream[0]
    fmas = [i for i, x in enumerate(ins) if x.startswith(("v_fmac_f64", "v_fma_f64"))]
    waits = [x for x in ins[:first] if x.startswith("s_waitcnt")]
    print("%-36s total %4d  VALU %4d  SALU %4d  VMEM %3d  SMEM %3d | before the stream %3d (waits: %s) | tail %3d | VGPRs %3d  SGPRs %3d  occupancy %d" %
          (name, len(ins), n["VALU"], n["SALU"], n["VMEM"], n["SMEM"], first, ", ".join(w.replace("s_waitcnt ", "") for w in waits) or "none",
           len(ins) - 1 - fmas[-1], meta.get("NumVgprs", -1), meta.get("NumSgprs", -1), meta.get("Occupancy", -1)))


def solve_report(name, body):
    ins = instrs(body)
    print(name)
    barrier = [i for i, x in enumerate(ins) if x.startswith("s_barrier")]
    marks = []
    for i, x in enumerate(ins):
        if x.startswith("s_load"):
            marks.append((i, x))
        elif x.startswith("s_barrier"):
            marks.append((i, x))
        elif re.match(r"global_load_\w+ .* nt", x) and not any("nt" in m[1] and m[1].startswith("global_load") for m in marks):
            marks.append((i, x + "      <- first tile load"))
    vm = [i for i, x in enumerate(ins) if x.startswith("global_load")]
    for i in vm[:6]:
        marks.append((i, ins[i] + "      <- vector load #%d of the kernel" % (vm.index(i) + 1)))
    for i, x in sorted(set(marks)):
        print("   %5d  %s" % (i, x))
    nt = next((i for i, x in enumerate(ins) if re.match(r"global_load_\w+ .* nt", x)), None)
    if nt is not None:
        b = max(j for j in barrier if j < nt)
        print("   between the barrier at %d and the first tile load at %d:" % (b, nt))
        for x in ins[b + 1:nt]:
            print("          " + x)


def main():
    lines = open(sys.argv[1]).read().split("\n")
    for name, prefix in PHI:
        _, body, meta = kernel_body(lines, prefix)
        phi_report(name, body, meta)
    _, body, _ = kernel_body(lines, SOLVE[1])
    solve_report(SOLVE[0], body)


if __name__ == "__main__":
    main()
