"""Instruction mix of the MFMA-bearing loops of a gfx950 assembly listing.

    hipcc <the flags of veles_amd/ops/build.py> --cuda-device-only -S \
        csrc/kernels/wgrad_halo.hip -o wgrad_halo.s
    python tools/isa_loop_mix.py wgrad_halo.s [kernel-name-substring]

For every kernel (whose mangled name holds the substring) it finds the loops
(a label and a later branch back to it) that hold MFMAs and are inside no
other such loop, and buckets their instructions by broad class, by mnemonic
prefix only: MFMA, VALU (and, of those, the quarter-rate integer multiplies
and 64-bit multiply-adds), SALU, branches, waits, LDS and buffer loads.
``saveexec`` counts the exec-masked regions opened in the loop.  The counts
are static (an inner scalar loop counts once).  Needs no GPU.

    python tools/isa_loop_mix.py --any ffn.s [substring]

takes the innermost loops with vector memory accesses instead, for kernels
without MFMAs (the element-wise passes: VALU per element = valu / the
elements a lane handles per turn).

    python tools/isa_loop_mix.py --waits wgrad_halo.s [substring]

reports instead, per loop, the ``s_waitcnt vmcnt`` instructions that stand
between an LDS-DMA issue (``buffer_load ... lds`` / ``global_load_lds``) and
the stage-end wait (the ``vmcnt(0)`` right in front of an ``s_barrier``):
the loop is cut into halves at its stage-end waits (a loop that runs two
pixel steps a turn has two), each half starting at its first DMA piece.  A
wait there holds the wave's LDS reads and MFMAs until its own pieces of the
NEXT stage have landed.  The other columns: LDS reads and MFMAs behind the
first piece, scratch accesses in the loop, and the kernel's VGPRs,
``.vgpr_spill_count``, ``.private_segment_fixed_size`` and LDS bytes.
"""
import re
import sys

QUARTER = ("v_mul_lo", "v_mul_hi", "v_mad_u64", "v_mad_i64")
COLS = ("mfma", "valu", "quarter", "salu", "branch", "wait", "lds", "buffer",
        "other", "saveexec")


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_cbranch") or op.startswith("s_branch"):
        return "branch"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("buffer_"):
        return "buffer"
    return "other"


def kernels(path):
    """[(name, vgprs, [(label | None, mnemonic, operands)])] per function"""
    out, cur, meta_name = [], None, None
    vg = {}
    global META
    with open(path) as f:
        for line in f:
            s = line.split(";")[0].rstrip()
            m = re.match(r"^(\w+):\s*$", s)
            if m and not s.startswith(".L"):
                name, cur = m.group(1), []
                out.append((name, cur))
                continue
            # metadata records list .name before .vgpr_count
            m = re.match(r"^\s*\.name:\s*(\S+)", line)
            if m:
                meta_name = m.group(1)
            m = re.match(r"^\s*\.vgpr_count:\s*(\d+)", line)
            if m and meta_name:
                vg[meta_name] = int(m.group(1))
            m = re.match(r"^\s*\.(vgpr_spill_count|private_segment_fixed_size"
                         r"|group_segment_fixed_size):\s*(\d+)", line)
            if m:   # (the two sizes precede .name in a record)
                if m.group(1) == "vgpr_spill_count":
                    if meta_name:
                        META.setdefault(meta_name, {}).update(PENDING)
                        META[meta_name][m.group(1)] = int(m.group(2))
                else:
                    PENDING[m.group(1)] = int(m.group(2))
            if cur is None:
                continue
            if s.startswith(".Lfunc_end"):
                cur = None
                continue
            m = re.match(r"^(\.LBB\w+):", s)
            if m:
                cur.append((m.group(1), None, None))
                continue
            m = re.match(r"^\s+([a-z]\w+)\s*(.*)$", s)
            if m and not m.group(1).startswith("."):
                cur.append((None, m.group(1), m.group(2)))
    return [(n, vg.get(n), body) for n, body in out]


def mfma_loops(body, any_loop=False):
    """the outermost loops that hold MFMAs; ``any_loop``: the INNERMOST loops
    with vector memory accesses instead (element-wise kernels)"""
    pos = {lab: i for i, (lab, _, _) in enumerate(body) if lab}
    loops = []
    for i, (lab, op, args) in enumerate(body):
        if op and (op.startswith("s_cbranch") or op.startswith("s_branch")):
            tgt = args.strip()
            if tgt in pos and pos[tgt] < i:
                seg = body[pos[tgt]:i + 1]
                want = ("global_", "buffer_") if any_loop else ("v_mfma",)
                if any(o and o.startswith(want) for _, o, _ in seg):
                    loops.append((pos[tgt], i))
    if any_loop:
        return [l for l in loops
                if not any(o != l and l[0] <= o[0] and o[1] <= l[1]
                           for o in loops)]
    # outermost only
    return [l for l in loops
            if not any(o != l and o[0] <= l[0] and l[1] <= o[1]
                       for o in loops)]


def mix(seg):
    c = dict.fromkeys(COLS, 0)
    for _, op, _ in seg:
        if not op:
            continue
        c[classify(op)] += 1
        if op.startswith(QUARTER):
            c["quarter"] += 1
        if "saveexec" in op:
            c["saveexec"] += 1
    return c


META, PENDING = {}, {}


def is_dma(op, args):
    return (op.startswith("buffer_load") and args.rstrip().endswith("lds")) \
        or op.startswith("global_load_lds")


def wait_halves(seg):
    """[(vmcnt waits, LDS reads, MFMAs) behind the first DMA piece] per loop
    half; halves end at a vmcnt(0) that an s_barrier follows."""
    ops = [(op, args) for _, op, args in seg if op]
    ends = []
    for i, (op, args) in enumerate(ops):
        if op == "s_waitcnt" and "vmcnt(0)" in args:
            nxt = [o for o, _ in ops[i + 1:i + 3]]
            if "s_barrier" in nxt:
                ends.append(i)
    if ends:   # the loop may be rotated: start behind its last stage end
        k = ends[-1] + 1
        ops = ops[k:] + ops[:k]
        ends = [(e - k) % len(ops) for e in ends]
    out, start = [], 0
    for e in ends + ([len(ops)] if not ends else []):
        half = ops[start:e]
        start = e + 1
        first = next((i for i, (o, a) in enumerate(half) if is_dma(o, a)),
                     None)
        if first is None:
            if any(o.startswith("v_mfma") for o, _ in half):
                out.append(None)   # a half without DMA
            continue
        tail = half[first:]
        out.append((
            [a.strip() for o, a in tail
             if o == "s_waitcnt" and "vmcnt" in a],
            sum(1 for o, _ in tail if o.startswith("ds_read")),
            sum(1 for o, _ in tail if o.startswith("v_mfma"))))
    return out


def main_waits(path, sub):
    print("| kernel | loop | half | vmcnt waits behind the first DMA piece | "
          "LDS reads | MFMAs | scratch in loop | VGPRs | spills | scratch "
          "bytes | LDS bytes |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for name, vgprs, body in kernels(path):
        if sub not in name:
            continue
        md = META.get(name, {})
        for k, (a, b) in enumerate(mfma_loops(body)):
            seg = body[a:b + 1]
            scr = sum(1 for _, op, _ in seg if op and op.startswith("scratch"))
            for h, r in enumerate(wait_halves(seg)):
                if r is None:
                    continue
                w, lds, mf = r
                if not (w or lds or mf):
                    continue   # only the DMA issue of the next turn
                print("| %s | %d | %d | %s | %d | %d | %d | %s | %s | %s | %s |"
                      % (name, k, h, ", ".join(w) if w else "none", lds, mf,
                         scr, vgprs, md.get("vgpr_spill_count"),
                         md.get("private_segment_fixed_size"),
                         md.get("group_segment_fixed_size")))


def main():
    if sys.argv[1] == "--waits":
        return main_waits(sys.argv[2], sys.argv[3] if len(sys.argv) > 3
                          else "")
    any_loop = sys.argv[1] == "--any"
    if any_loop:
        del sys.argv[1]
    path = sys.argv[1]
    sub = sys.argv[2] if len(sys.argv) > 2 else ""
    print("| kernel | loop | " + " | ".join(COLS) + " | VGPRs |")
    print("|---|---|" + "---|" * (len(COLS) + 1))
    for name, vgprs, body in kernels(path):
        if sub not in name:
            continue
        for k, (a, b) in enumerate(mfma_loops(body, any_loop)):
            c = mix(body[a:b + 1])
            print("| %s | %d | %s | %s |" % (
                name, k, " | ".join(str(c[x]) for x in COLS), vgprs))


if __name__ == "__main__":
    main()
