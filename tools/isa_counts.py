#!/usr/bin/env python3
"""Instruction counts of the built forward kernel (latency build), read off its ISA: what
tools/chain_floor.py's table of dependent operations is checked against, and what the register
allocator had to do to fit the kernel (spills into vector lanes / accumulation registers).

Compiles peakseg_hip.cpp for the device only (-S), takes psd::lat::fpop_forward_kernel and prints
  * resource usage (registers, scratch, LDS),
  * instructions by class over the whole kernel (hot and cold blocks together),
  * the Newton loops: innermost loops that contain two / one f64 divisions and a table look-up
    (get_larger_root: a log and two divisions per trip; get_smaller_root: an exp and one), with
    their instruction counts per trip.

With --phases the stamped diagnostic build (-DPSD_PROFILE, line tables on) is compiled as well
and its per-data-point code is split at the cycle stamps (PSD_PROF_T0 / PSD_PROF_ADD /
PSD_PROF_SUB in the sources): per phase, the static number of branches, of exec-mask regions
(s_*_saveexec), of s_cbranch_execz skips, of s_waitcnt and of SALU / VALU instructions, counted
in layout order between two stamps (the fall-through path and the blocks the compiler laid out
inside it; out-of-line cold blocks are listed under the phase whose stamp follows them).

With --loop-paths the two ends of the usual data point (loop top, end of the data point) are
measured as shortest paths through the kernel's control-flow graph, for this tree and for any
other source trees named after the flag (a checkout of the parent commit, say).

usage: python tools/isa_counts.py [--phases] [out.txt]   (no GPU needed)
       python tools/isa_counts.py --loop-paths [other-tree ...]
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

KERNEL = "_ZN3psd3lat19fpop_forward_kernelENS_10DeviceArgsE"


def stamp_sites(csrc):
    """{(file name, line): label} of every cycle stamp in the kernel sources."""
    sites = {}
    for name in os.listdir(csrc):
        for no, ln in enumerate(open(os.path.join(csrc, name), errors="replace"), 1):
            m = re.search(r"\bPSD_PROF_(T0|SUB0|ADD|SUB)\((\w*)\)", ln)
            if m and not ln.lstrip().startswith("#define"):
                sites[(name, no)] = m.group(2) if m.group(1) in ("ADD", "SUB") else "(start)"
    return sites


def phase_table(csrc, work):
    """Static counts per phase of the stamped build, split at the cycle-counter reads."""
    asm = os.path.join(work, "prof.s")
    flags = [f for f in entry.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([entry.HIPCC] + flags + ["--cuda-device-only", "-S", "-DPSD_PROFILE",
                    "-gline-tables-only", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                    os.path.join(csrc, "peakseg_hip.cpp"), "-o", asm], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(asm).read()
    files = {int(m.group(1)): os.path.basename(m.group(3) or m.group(2)) for m in
             re.finditer(r'\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', text)}
    start = text.index("\n" + KERNEL + ":")
    body = text[start:text.index(".end_amdhsa_kernel", start)]
    sites = stamp_sites(csrc)
    keys = ("branches", "execz skips", "exec regions", "s_waitcnt", "SALU", "VALU", "LDS", "all")
    order, table = [], {}
    pending = dict.fromkeys(keys, 0)
    loc = None
    for ln in body.splitlines():
        t = ln.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            loc = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        i = t.split(";")[0].strip()
        if not i or i.startswith(".") or i.endswith(":"):
            continue
        if i.startswith(("s_memtime", "s_memrealtime")) and loc in sites:
            label = "%s @ %s:%d" % (sites[loc], loc[0], loc[1])
            if label not in table:
                order.append(label)
                table[label] = dict.fromkeys(keys, 0)
            for k in keys:
                table[label][k] += pending[k]
            pending = dict.fromkeys(keys, 0)
            continue
        pending["all"] += 1
        pending["branches"] += i.startswith(("s_cbranch", "s_branch"))
        pending["execz skips"] += i.startswith("s_cbranch_exec")
        pending["exec regions"] += "saveexec" in i
        pending["s_waitcnt"] += i.startswith("s_waitcnt")
        pending["SALU"] += i.startswith("s_")
        pending["VALU"] += i.startswith("v_")
        pending["LDS"] += i.startswith("ds_")
    out = ["static counts per phase of the stamped build (instructions in layout order up to each "
           "stamp; '(start)' rows: code between the end of one phase and the start of the next):",
           "  %-46s" % "stamp" + "".join("%13s" % k for k in keys)]
    for label in order:
        out.append("  %-46s" % label + "".join("%13d" % table[label][k] for k in keys))
    out.append("  %-46s" % "(after the last stamp)" + "".join("%13d" % pending[k] for k in keys))
    return out


TOP_ANCHORS = [r"const int n_own = uniform_i\(g_sm\.n\[2 \* chain \+ b\]\);",  # the inner loop's top
               r"if \(\(t & 63\) == 0 \|\| t == t_first\)"]                    # (before it existed)
STATUS_ANCHOR = r"status = uniform_i\(g_sm\.abort_status\[slot\]\);"


def loop_paths(root, work):
    """The two ends of the usual data point in the latency kernel of the source tree `root`, as
    shortest paths through the kernel's control-flow graph (one step per instruction; a skip
    over an exec-mask region, s_cbranch_execz, counts as not taken):
      top:    from the first instruction of the data-point loop (the inner loop of the usual data
              point where the tree has one) to the first LDS read of the first pass;
      bottom: from the read of the barrier's status word (right after step_sync) to the loop's
              first instruction again.
    The shortest path is the one without the 64-point data load, errors or cold calls, i.e. what
    63 of 64 usual data points execute.  Per path: instructions, spill stores (v_writelane of a
    scalar), spill reloads (v_readlane from a spill register), v_accvgpr moves, uniform
    conditions made into 64-bit masks (s_cselect_b64 -1, 0), branches through vcc / through scc.
    Also says where the data-point counter lives (the register incremented at the t++)."""
    import heapq
    csrc = os.path.join(root, "peaksegdisk_amd", "csrc")
    asm = os.path.join(work, "loop.s")
    flags = [f for f in entry.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([entry.HIPCC] + flags + ["--cuda-device-only", "-S", "-gline-tables-only",
                    "-I" + os.path.join(root, "include"), "-I" + csrc,
                    os.path.join(csrc, "peakseg_hip.cpp"), "-o", asm], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(asm).read()
    files = {int(m.group(1)): os.path.basename(m.group(3) or m.group(2)) for m in
             re.finditer(r'\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', text)}
    start = text.index("\n" + KERNEL + ":")
    body = text[start:text.index(".end_amdhsa_kernel", start)]
    src = open(os.path.join(csrc, "fpop_kernels.h")).read().splitlines()

    def src_line(patterns):
        for pat in patterns:
            hits = [no for no, ln in enumerate(src, 1) if re.search(pat, ln)]
            if hits:
                return hits[0]
        raise SystemExit("anchor not found in fpop_kernels.h: %r" % (patterns,))
    top_line, status_line = src_line(TOP_ANCHORS), src_line([STATUS_ANCHOR])
    insts, locs, label_at = [], [], {}
    loc = None
    for ln in body.splitlines():
        t = ln.split(";")[0].strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            loc = (files.get(int(m.group(1)), "?"), int(m.group(2)))
        elif t.endswith(":"):
            label_at[t[:-1]] = len(insts)
        elif t and not t.startswith("."):
            insts.append(t)
            locs.append(loc)
    spill_regs = {m.group(1) for i in insts
                  for m in [re.match(r"v_writelane_b32 (v\d+), s\d+, \d+", i)] if m}

    def succ(k):
        i = insts[k]
        m = re.match(r"s_c?branch\w*\s+(\S+)", i)
        out = []
        if m and not i.startswith("s_cbranch_execz"):
            out.append(label_at[m.group(1)])
        if not i.startswith(("s_branch", "s_endpgm", "s_setpc")) and k + 1 < len(insts):
            out.append(k + 1)
        return out

    def shortest(a, goal):
        dist, prev, heap = {a: 0}, {}, [(0, a)]
        while heap:
            d, k = heapq.heappop(heap)
            if goal(k) and k != a:
                path = [k]
                while path[-1] != a:
                    path.append(prev[path[-1]])
                return path[::-1][:-1]  # (the instruction at the goal belongs to what follows)
            if d > dist[k]:
                continue
            for n in succ(k):
                if n not in dist or d + 1 < dist[n]:
                    dist[n], prev[n] = d + 1, k
                    heapq.heappush(heap, (d + 1, n))
        raise SystemExit("no path")
    first_of = lambda line: min(k for k, l in enumerate(locs) if l == ("fpop_kernels.h", line))
    header = first_of(top_line)
    # (the loop's first instruction: back to the start of the block the anchor's line begins)
    status = min(k for k, l in enumerate(locs) if l == ("fpop_kernels.h", status_line) and k > header)
    first_pass = lambda k: insts[k].startswith("ds_read") and locs[k] and \
        locs[k][0] not in ("fpop_kernels.h", "psd_platform.h")
    # the way back to the header goes through the increment of the data-point counter (the
    # shortest path as such would leave the loop as if with an error and enter it again): the
    # add of 1 to a register that is also masked with 63 (the lane of the data block)
    lane_regs = {m.group(1) or m.group(2) for i in insts for m in
                 [re.match(r"(?:s_and_b32 \S+ (s\d+), 63$|v_and_b32\w* \S+ 63, (v\d+)$)", i)] if m}
    incs = [k for k, i in enumerate(insts) for m in
            [re.match(r"(?:s_add_i32 (s\d+), \1, 1$|v_add_u32\w* (v\d+), 1, \2$)", i)]
            if m and (m.group(1) or m.group(2)) in lane_regs]
    best = None
    for inc in incs:
        try:
            way = shortest(status, lambda k: k == inc) + shortest(inc, lambda k: k == header)
        except SystemExit:
            continue
        if best is None or len(way) < len(best[1]):
            best = (inc, way)
    paths = (("top: loop header -> first LDS read of the first pass", shortest(header, first_pass)),
             ("bottom: status word read after step_sync -> t++ -> loop header", best[1]))
    out = ["the two ends of the usual data point (%s), shortest paths through the kernel's CFG:"
           % os.path.basename(os.path.abspath(root))]
    keys = ("instructions", "spill stores", "spill reloads", "v_accvgpr", "v_mov",
            "conditions as masks", "vcc branches", "scc branches")
    for name, path in paths:
        p = [insts[k] for k in path]
        n = dict.fromkeys(keys, 0)
        n["instructions"] = len(p)
        for i in p:
            n["spill stores"] += bool(re.match(r"v_writelane_b32 v\d+, s\d+, \d+", i))
            m = re.match(r"v_readlane_b32 s\d+, (v\d+), \d+", i)
            n["spill reloads"] += bool(m and m.group(1) in spill_regs)
            n["v_accvgpr"] += i.startswith("v_accvgpr")
            n["v_mov"] += i.startswith("v_mov")
            n["conditions as masks"] += bool(re.match(r"s_cselect_b64 \S+ -1, 0", i))
            n["vcc branches"] += i.startswith("s_cbranch_vcc")
            n["scc branches"] += i.startswith("s_cbranch_scc")
        out.append("  " + name)
        out.append("    " + ", ".join("%s %d" % (k, n[k]) for k in keys))
    # the data-point counter: the add of 1 on the path from the status word back to the header
    out.append("  the data-point counter's increment: %s  (%s register)"
               % (insts[best[0]], "a scalar" if insts[best[0]].startswith("s_") else "a vector"))
    return out


def main():
    phases = "--phases" in sys.argv
    if phases:
        sys.argv.remove("--phases")
    if "--loop-paths" in sys.argv:
        # usage: isa_counts.py --loop-paths [other source tree ...] : this tree, then the others
        k = sys.argv.index("--loop-paths")
        work = tempfile.mkdtemp(prefix="psd_isa_")
        lines = []
        for root in [ROOT] + sys.argv[k + 1:]:
            lines += loop_paths(root, work)
        sys.stdout.write("\n".join(lines) + "\n")
        return
    csrc = os.path.join(ROOT, "peaksegdisk_amd", "csrc")
    work = tempfile.mkdtemp(prefix="psd_isa_")
    asm = os.path.join(work, "dev.s")
    flags = [f for f in entry.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([entry.HIPCC] + flags + ["--cuda-device-only", "-S",
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                    os.path.join(csrc, "peakseg_hip.cpp"), "-o", asm], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(asm).read()
    start = text.index("\n" + KERNEL + ":")
    end = text.index(".end_amdhsa_kernel", start)
    body = text[start:end]
    lines = [ln.split(";")[0].strip() for ln in body.splitlines()]  # (comments follow a ';')
    insts = [ln for ln in lines if ln and not ln.startswith((".", ";")) and not ln.endswith(":")]
    out = []
    out.append("psd::lat::fpop_forward_kernel (%s), %s" % (
        " ".join(f for f in entry.HIP_FLAGS if f.startswith("-O") or f.startswith("-f")), "gfx950"))
    for key in ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size",
                "group_segment_fixed_size"):
        m = re.search(r"\.amdhsa_%s (\d+)" % key, body)
        if m:
            out.append("  %-28s %s" % (key, m.group(1)))
    for key in ("sgpr_spill_count", "vgpr_spill_count"):
        m = re.search(r"\.name:\s+%s.*?\.%s:\s+(\d+)" % (KERNEL, key), text, re.S)
        if m:
            out.append("  %-28s %s" % (key, m.group(1)))
    classes = [
        ("all instructions", lambda i: True),
        ("VALU (v_*)", lambda i: i.startswith("v_")),
        ("  f64 arithmetic", lambda i: re.match(r"v_(fma|fmac|mul|add|div_\w+|rcp|min|max)_f64", i)),
        ("  divisions (v_rcp_f64)", lambda i: i.startswith("v_rcp_f64")),
        ("  v_readlane / v_writelane", lambda i: i.startswith(("v_readlane", "v_writelane"))),
        ("  v_accvgpr_read / write (VGPR spills to AGPRs)", lambda i: i.startswith("v_accvgpr")),
        ("SALU (s_*)", lambda i: i.startswith("s_")),
        ("  branches", lambda i: i.startswith(("s_cbranch", "s_branch"))),
        ("    s_cbranch_execz / execnz", lambda i: i.startswith("s_cbranch_exec")),
        ("  exec-mask regions (s_*_saveexec)", lambda i: "saveexec" in i),
        ("  s_waitcnt", lambda i: i.startswith("s_waitcnt")),
        ("  calls (s_swappc)", lambda i: i.startswith("s_swappc")),
        ("LDS reads (ds_read*)", lambda i: i.startswith("ds_read")),
        ("LDS writes (ds_write*)", lambda i: i.startswith("ds_write")),
        ("LDS other (ds_bpermute, ds_add, ...)", lambda i: i.startswith("ds_") and not i.startswith(("ds_read", "ds_write"))),
        ("global loads", lambda i: i.startswith("global_load")),
        ("global stores", lambda i: i.startswith("global_store")),
        ("scratch (register spills to memory)", lambda i: i.startswith("scratch_")),
    ]
    out.append("instructions in the kernel's body (hot and cold blocks):")
    for name, pred in classes:
        out.append("  %-50s %6d" % (name, sum(1 for i in insts if pred(i))))
    # innermost loops: a label, then a backward branch to it with no other label in between
    out.append("Newton loops (innermost loops with f64 divisions and a table look-up):")
    label_at = {}
    seq = []
    for ln in lines:
        if ln.endswith(":") and ln.startswith(".LBB"):
            label_at[ln[:-1]] = len(seq)
        elif ln and not ln.startswith((".", ";")):
            seq.append(ln)
    labels_sorted = sorted(label_at.items(), key=lambda kv: kv[1])
    for name, at in labels_sorted:
        nxt = min([a for _, a in labels_sorted if a > at] + [len(seq)])
        block = seq[at:nxt]
        back = [k for k, i in enumerate(block) if re.match(r"s_cbranch_\w+\s+%s\b" % re.escape(name), i)]
        if not back:
            continue
        block = block[:back[0] + 1]
        n_div = sum(1 for i in block if i.startswith("v_rcp_f64"))
        n_lds = sum(1 for i in block if i.startswith("ds_read"))
        if n_div == 0 or n_lds == 0:
            continue
        kind = "larger root (log, two divisions)" if n_div == 2 else "smaller root (exp, one division)"
        out.append("  %-12s %-36s %3d instructions per trip: %d VALU, %d SALU, %d LDS" % (
            name, kind, len(block), sum(1 for i in block if i.startswith("v_")),
            sum(1 for i in block if i.startswith("s_")), n_lds))
    if phases:
        out += phase_table(csrc, work)
    text_out = "\n".join(out) + "\n"
    sys.stdout.write(text_out)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text_out)


if __name__ == "__main__":
    main()
