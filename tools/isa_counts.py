#!/usr/bin/env python3
"""
Static instruction counts of the evaluation step's kernels from a device listing of csrc/plan.hip:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Iinclude -Ibluest_amd/csrc \
          -mllvm -amdgpu-kernarg-preload-count=16 bluest_amd/csrc/plan.hip -o plan.s      (the unit's flags of bluest_amd/build.py)
    python tools/isa_counts.py plan.s [--paths]      (--paths: every instruction in front of the first stream / fold load)

Per Phi kernel: all instructions of the listing (every block once -- which is what a wavefront executes when iters = 1 and
n_cand = 1, minus the block a branch skips), split into VALU / SALU / VMEM / SMEM, the instructions in front of the first
streaming load, those behind the loop's last FMA (the tail), the waits in front of the stream, the registers and the number of
argument dwords the descriptor has preloaded into scalar registers (kernarg preload); then the loads, barriers and waits from the
entry to the first streaming load.  A kernel with preloaded arguments is read from its preload entry (preload_entry).
For k_solve_grad<20,5>: the instruction counts of four regions (solve_regions: entry -> first fold load along the shortest path,
the fold, the tile stream and the solving wavefront between the barriers, the tile wavefronts behind the second barrier) and the
registers, with the loads, barriers and waits along the path of region (1); then the line numbers (relative to the kernel's start,
in the order of the text) of the descriptor load, the late kernarg loads, the
first load of the fold, the barriers and the first non-temporal tile load, with the waits between the first barrier and that load.
"""
import re
import sys

# (prefixes of the mangled names: the argument lists may change)
PHI = [("k_phi_chunks_shared<%d,1,uint16_t>" % ob, "_Z19k_phi_chunks_sharedILi%dELi1EtE" % ob) for ob in (2, 4, 8)]
PHI.append(("k_phi_chunks<1,uint16_t>", "_Z12k_phi_chunksILi1EtE"))
SOLVE = ("k_solve_grad<20,5>", "_Z12k_solve_gradILi20ELi5EE")


def kernel_body(lines, prefix):
    start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and l.split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    meta = {}
    for l in lines[end:end + 120]:
        m = re.match(r"\s*;\s*(NumVgprs|NumSgprs|TotalNumSgprs|Occupancy|ScratchSize|NumAgprs):\s*(\d+)", l)
        if m:
            meta[m.group(1)] = int(m.group(2))
    meta.setdefault("NumSgprs", meta.get("TotalNumSgprs", -1))
    meta["Preload"] = 0
    for l in lines[start:end]:      # the kernel descriptor stands between s_endpgm and .Lfunc_end
        m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", l)
        if m:
            meta["Preload"] = int(m.group(1))
    body = [l for l in lines[start + 1:end + 1]]
    return start, body[preload_entry(body):], meta


def preload_entry(body):
    """A kernel with preloaded arguments (kernarg preload, descriptor field preload_length > 0) begins with a prologue for firmware
    without the feature: it loads those arguments from the argument segment, waits and branches to the entry proper, the block
    behind the next `.p2align 8`, where a wavefront whose arguments were preloaded starts.  Index of that block's first line
    (0: no prologue); every count and every "from the kernel's entry" below starts there."""
    for i, l in enumerate(body[:40]):
        t = l.strip()
        if re.match(r"\.p2align\s+8", t):
            return i + 1
        if t and not t.startswith((";", "s_load_dword", "s_waitcnt", "s_branch", "s_nop")):
            break
    return 0


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
    print("%-36s total %4d  VALU %4d  SALU %4d  VMEM %3d  SMEM %3d | before the stream %3d (waits: %s) | tail %3d | VGPRs %3d  SGPRs %3d  occupancy %d  preload %d" %
          (name, len(ins), n["VALU"], n["SALU"], n["VMEM"], n["SMEM"], first, ", ".join(w.replace("s_waitcnt ", "") for w in waits) or "none",
           len(ins) - 1 - fmas[-1], meta.get("NumVgprs", -1), meta.get("NumSgprs", -1), meta.get("Occupancy", -1), meta["Preload"]))


def entry_report(name, body):
    """loads, barriers and waits of a Phi kernel from its entry to the first load of the stream"""
    ins = instrs(body)
    first = next(i for i, x in enumerate(ins) if re.match(r"global_load_dwordx(2|4)", x))
    print(name)
    for i, x in enumerate(ins[:first + 1]):
        if PATHS or x.startswith(("s_load", "s_buffer_load", "global_load", "s_barrier", "s_waitcnt")):
            print("   %5d  %s%s" % (i, x, "      <- first load of the stream" if i == first else ""))


def first_fold_load(text):
    """index of the regular fold's first partial load in a list of instructions: the rank_ab load (the kernel's first
    global_load_ushort) belongs to the same row; the first 16-byte load behind it, or -- a kernel that issues the partials' loads in
    front of it -- the earliest 16-byte load in front of it with no barrier and no LDS operation in between"""
    ush = next(i for i, x in enumerate(text) if x.startswith("global_load_ushort"))
    first = None
    for i in range(ush - 1, -1, -1):
        if text[i].startswith(("s_barrier", "ds_")):
            break
        if text[i].startswith("global_load_dwordx4"):
            first = i
    return first if first is not None else next(i for i in range(ush, len(text)) if text[i].startswith("global_load_dwordx4"))


def solve_report(name, body):
    ins = instrs(body)
    print(name)
    barrier = [i for i, x in enumerate(ins) if x.startswith("s_barrier")]
    fold = first_fold_load(ins)
    marks = [(fold, ins[fold] + "      <- first partial load of the regular fold")]
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


def blocks_of(body):
    """basic blocks of a kernel's text: list of (labels, [instructions]); a block ends behind a branch or s_endpgm, or in front of a label"""
    out, labels, cur = [], [], []
    for l in body:
        t = l.strip()
        m = re.match(r"^([.\w$]+):", t)
        if m:
            if cur:
                out.append((labels, cur))
                labels, cur = [], []
            labels.append(m.group(1))
            continue
        if not t or t.startswith((";", ".", "//")):
            continue
        ins = t.split(";")[0].strip()
        cur.append(ins)
        if ins.startswith(("s_cbranch", "s_branch", "s_endpgm")):
            out.append((labels, cur))
            labels, cur = [], []
    if cur:
        out.append((labels, cur))
    return out


def tally(ins):
    n = {k: 0 for k in ("VALU", "SALU", "VMEM", "SMEM", "LDS")}
    for i in ins:
        n[kind(i)] += 1
    return "%4d  (VALU %4d  SALU %4d  VMEM %3d  SMEM %2d  LDS %3d)" % (len(ins), n["VALU"], n["SALU"], n["VMEM"], n["SMEM"], n["LDS"])


def solve_regions(name, body, meta):
    """k_solve_grad in four regions.  (1) entry -> the regular fold's first partial load: the SHORTEST path through the kernel's
    blocks that meets no vector load, LDS operation or barrier on its way -- what a wavefront of a plan without a gate, with equal
    workgroups per output, no pads and no record executes.  (2) the fold: the text from that load to the barrier behind it, every
    instruction once (all eight slot counts of the regular fold are in it; a wavefront runs one of them; in a kernel that issues
    the fold's loads at its entry the gate, line-search and pad-clearing blocks stand in it too).  (3) between that barrier
    and the next: the tile wavefronts' stream (up to the last 16-byte load) and the solving wavefront (the rest: every pass and
    rare path of solve_wave once).  (4) behind the second barrier: the tile wavefronts' forms and stores, all group sizes."""
    bl = blocks_of(body)
    flat = [(b, j) for b, (_, ins) in enumerate(bl) for j in range(len(ins))]
    text = [bl[b][1][j] for b, j in flat]
    first = first_fold_load(text)
    tb, tj = flat[first]
    label_block = {lab: b for b, (labs, _) in enumerate(bl) for lab in labs}
    clean = lambda ins: not any(x.startswith(("global_", "flat_", "buffer_", "ds_", "s_barrier")) and      # noqa: E731
                                not x.startswith("global_load_ushort") for x in ins)      # (the row's rank_ab load belongs to the fold)
    # shortest path over blocks, cost = instructions executed
    import heapq
    dist, heap = {0: 0}, [(0, 0, [0])]
    best = None
    while heap:
        d, b, path = heapq.heappop(heap)
        if b == tb:
            best = (d, path)
            break
        if d > dist.get(b, 1 << 30) or not clean(bl[b][1]):
            continue
        ins = bl[b][1]
        last = ins[-1]
        succ = []
        if last.startswith("s_endpgm"):
            continue
        if last.startswith(("s_branch", "s_cbranch")):
            succ.append(label_block[last.split()[-1]])
        if not last.startswith("s_branch") and b + 1 < len(bl):
            succ.append(b + 1)
        for nb in succ:
            nd = d + len(ins)
            if nd < dist.get(nb, 1 << 30):
                dist[nb] = nd
                heapq.heappush(heap, (nd, nb, path + [nb]))
    print(name + "   VGPRs %d  SGPRs %d  scratch %d  occupancy %d  preload %d" % (meta.get("NumVgprs", -1), meta.get("NumSgprs", -1),
                                                                                 meta.get("ScratchSize", -1), meta.get("Occupancy", -1), meta["Preload"]))
    if best is None:
        print("   (1) entry -> first fold load: no path without a vector load, an LDS operation or a barrier")
    else:
        head = [x for b in best[1][:-1] for x in bl[b][1]] + bl[tb][1][:tj]
        print("   (1) entry -> first fold load        %s   waits on the way: %s" % (
            tally(head), ", ".join(x.replace("s_waitcnt ", "") for x in head if x.startswith("s_waitcnt")) or "none"))
        print("       loads, barriers and waits on that path (numbered along the path):")
        for i, x in enumerate(head):
            if PATHS or x.startswith(("s_load", "s_buffer_load", "global_load", "s_barrier", "s_waitcnt")):
                print("          %4d  %s" % (i, x))
    bar =[i for i, x in enumerate(text) if x.startswith("s_barrier")]
    b1, b2 = bar[-2], bar[-1]      # (the kernel's last two barriers: behind the fold, and behind the solve; earlier ones belong to the gate and the pads)
    print("   (2) fold, first load -> barrier      %s" % tally(text[first:b1]))
    tl = max(i for i in range(b1, b2) if text[i].startswith("global_load_dwordx4"))
    print("   (3) tile stream behind the barrier   %s" % tally(text[b1 + 1:tl + 1]))
    print("       solving wavefront -> 2nd barrier %s" % tally(text[tl + 1:b2]))
    print("   (4) behind the second barrier        %s" % tally(text[b2 + 1:]))
    print("       whole kernel                     %s" % tally(text))


PATHS = False      # --paths: every instruction in front of the first stream / fold load, not only the loads, barriers and waits


def main():
    global PATHS
    PATHS = "--paths" in sys.argv[2:]
    lines = open(sys.argv[1]).read().split("\n")
    for name, prefix in PHI:
        _, body, meta = kernel_body(lines, prefix)
        phi_report(name, body, meta)
    for name, prefix in PHI:
        entry_report(name, kernel_body(lines, prefix)[1])
    _, body, meta = kernel_body(lines, SOLVE[1])
    solve_regions(SOLVE[0], body, meta)
    solve_report(SOLVE[0], body)


if __name__ == "__main__":
    main()
