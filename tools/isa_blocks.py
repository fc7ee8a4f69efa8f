#!/usr/bin/env python3
"""Splits a kernel's gfx950 assembly (hipcc -S) into basic blocks and counts instruction classes per block:
   python3 tools/isa_blocks.py file.s [kernel-substring]
Prints label, line, #VALU (and how many are half-rate / transcendental by the calibration table of DESIGN 5b), #SALU,
#VMEM, #LDS, #branches and the branch targets - enough to attribute a kernel's instruction budget to its source blocks.

   python3 tools/isa_blocks.py --routes file.s kernel-substring [classes, e.g. 13,14,9,10,8,11,9,10,5,4,7,6]
The exact PLAIN pass's class switch (ptk_kernels.hip; DESIGN 4.1 "The pass"): for each of the sixteen zero classes the static route
from the pass loop's header to the join - the first instruction every class executes behind its body, where the accept chain
starts - followed by interpreting the scalar compares, flag moves and flag tests along it.  Per class: scalar ALU instructions,
conditional branches (and how many are taken), unconditional branches, flag-test hops (an s_cbranch_vcc* fed by
s_andn2_b64 / s_and_b64 vcc, exec, <flag>) and VALU; with a class list, the sums over it (one pass of a scene with those records).
Also checks the kernel's control flow: every s_and_saveexec_b64 is closed by an s_or_b64 exec on every route (check_exec_regions)
and lists the natural loops with their back edges and exits (loops).  On a kernel of the pair unit (csrc/ptk_kernels_rect.hip) the
pair loop in front of the record loop is walked the same way, per kind 1..6 (pair_header, route_table(K, pair_header(K), range(1, 7))).
--routes also prints deal_route: what lies between the pass's latch and the shade block on the route of one deal of one round."""
import re, sys
HALF = re.compile(r"^v_(cmp|cmpx|cndmask|min|max|med3|cvt|bfe|perm|and_or|mad_u32|mul_lo|mul_hi|lshl_add|lshl_or|add_lshl|div_|pk_|bfi|alignbit|sad|mad_i32|mad_u64|add3|xad|or3|readlane|readfirstlane|writelane|ldexp|frexp|fract|trunc|floor|rndne|ceil)")
TRANS = re.compile(r"^v_(rcp|sqrt|rsq|exp|log|sin|cos)")
LABEL = re.compile(r"^(\.LBB[\w]+|[A-Za-z_][\w.$]*):")


def blocks_of(path, want):
    lines = open(path).read().split("\n")
    blocks = []; cur = None; active = want is None
    for i, l in enumerate(lines):
        s = l.strip()
        if re.match(r"^[A-Za-z_.$][\w.$]*:", s) and not s.startswith(".L") and want:
            active = want in s
        if not active: continue
        m = LABEL.match(s)
        if m:
            cur = dict(label=m.group(1), line=i + 1, valu=0, half=0, trans=0, salu=0, vmem=0, lds=0, smem=0, br=[], wait=0); blocks.append(cur); continue
        if cur is None or not s or s.startswith(";") or s.startswith("."): continue
        op = s.split()[0]
        if op.startswith("v_"):
            cur["valu"] += 1
            if TRANS.match(op): cur["trans"] += 1
            elif HALF.match(op): cur["half"] += 1
        elif op.startswith("s_cbranch") or op == "s_branch":
            cur["br"].append(op.replace("s_cbranch_", "") + ">" + s.split()[-1]); cur["salu"] += 1
        elif op.startswith("s_waitcnt"): cur["wait"] += 1
        elif op.startswith("s_load") or op.startswith("s_buffer"): cur["smem"] += 1
        elif op.startswith("s_"): cur["salu"] += 1
        elif op.startswith("global_") or op.startswith("buffer_") or op.startswith("flat_") or op.startswith("scratch_"): cur["vmem"] += 1
        elif op.startswith("ds_"): cur["lds"] += 1
    return blocks


# ---- the kernel as an instruction list ---------------------------------------------------------------------------------------
class Kernel:
    """ins: [(source line, opcode, [operands])] of one kernel of a hipcc -S file; label: name -> index of the instruction it precedes"""
    def __init__(self, path, want):
        self.ins = []; self.label = {}; self.meta = {}
        active = False; name = None
        for i, l in enumerate(open(path).read().split("\n")):
            s = l.strip()
            m = LABEL.match(s)
            if m and not s.startswith(".L"):
                active = want in s and s.startswith("_Z")
                if active: name = m.group(1)
            if s.startswith(".end_amdhsa_kernel") or s.startswith(".Lfunc_end"): active = False
            if not active: continue
            if m:
                self.label[m.group(1)] = len(self.ins); continue
            s = s.split(";")[0].strip()
            if not s or s.startswith("."): continue
            parts = s.split(None, 1)
            ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
            self.ins.append((i + 1, parts[0], ops))
        assert name, "no kernel matches " + want
        self.name = name
        # the kernel's metadata record (registers, spills, scratch)
        txt = open(path).read()
        k = txt.find("amdhsa.kernels:")
        for rec in re.split(r"\n  - ", txt[k:]) if k >= 0 else []:
            if not re.search(r"\.name:\s+" + re.escape(name) + r"\s", rec): continue
            for key in ("private_segment_fixed_size", "vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "max_flat_workgroup_size"):
                m = re.search(r"\." + key + r":\s+(\d+)", rec)
                if m: self.meta[key] = int(m.group(1))

    def targets(self, i):
        """(successors of instruction i, its kind)"""
        _, op, ops = self.ins[i]
        if op == "s_branch": return [self.label[ops[0]]], "branch"
        if op.startswith("s_cbranch_"): return [i + 1, self.label[ops[0]]], "cbranch"
        if op == "s_endpgm": return [], "end"
        return [i + 1], ""


def _imm(x):
    try: return int(x, 0)
    except ValueError: return None


def _sregs(o):
    m = re.match(r"^s\[(\d+):(\d+)\]$", o)
    if m: return ["s%d" % k for k in range(int(m.group(1)), int(m.group(2)) + 1)]
    return [o] if re.match(r"^(s\d+|vcc|vcc_lo|vcc_hi|exec)$", o) else []


def nibble_headers(K):
    """every loop that extracts a nibble per turn (s_lshr_b64 + s_and_b32 ..., 15), in program order: (index of the loop's first
    instruction, index of the extraction, the register that receives the nibble)"""
    out = []
    for i, (_, op, ops) in enumerate(K.ins):
        if op == "s_and_b32" and len(ops) == 3 and ops[2] == "15" and i > 0 and K.ins[i - 1][1] == "s_lshr_b64":
            out.append((max(v for v in K.label.values() if v <= i), i, ops[0]))
    return out


def pass_header(K):
    """index of the record loop's first instruction and the register that receives the class nibble (the last such loop of the
    kernel: in the pair unit, csrc/ptk_kernels_rect.hip, the pair loop stands in front of it)"""
    hs = nibble_headers(K)
    if not hs: raise AssertionError("no class extraction (s_lshr_b64 + s_and_b32 ..., 15) in " + K.name)
    return hs[-1]


def pair_header(K):
    """... and the pair loop's: the kind nibble of a pair of records (kernels of the pair unit only)"""
    hs = nibble_headers(K)
    if len(hs) != 2: raise AssertionError("%d nibble loops in %s: not a kernel of the pair unit" % (len(hs), K.name))
    return hs[0]


CMP = {"lt": lambda a, b: a < b, "gt": lambda a, b: a > b, "le": lambda a, b: a <= b, "ge": lambda a, b: a >= b,
       "eq": lambda a, b: a == b, "lg": lambda a, b: a != b}


def route(K, cls, header=None):
    """(header: pass_header(K), the default, or pair_header(K) with cls = the pair's kind) the instructions a wave executes from the pass loop's header until it is back there (or leaves the loop) for a record of class
    `cls`, every lane in TRAV and some lane accepting (execz branches not taken): [(index, taken or None)], and the flag-test hops"""
    h, at, creg = header or pass_header(K)
    val = {}           # scalar registers with a known value; 64-bit flags under the name of their first operand text
    scc = None; vcc = None; vcc_from_flag = False
    out = []; hops = []
    i = h
    for _ in range(4000):
        line, op, ops = K.ins[i]
        taken = None
        nxt = i + 1
        if i == at: val = {creg: cls}
        elif op.startswith("s_cmp_") and op[6:8] in CMP:
            a = val.get(ops[0], _imm(ops[0])); b = val.get(ops[1], _imm(ops[1]))
            scc = None if a is None or b is None else CMP[op[6:8]](a, b)
        elif op in ("s_bitcmp1_b32", "s_bitcmp0_b32"):
            a = val.get(ops[0]); b = _imm(ops[1])
            scc = None if a is None or b is None else (((a >> b) & 1) == (1 if op == "s_bitcmp1_b32" else 0))
        elif op in ("s_mov_b64", "s_mov_b32"):
            v = val.get(ops[1], _imm(ops[1]))
            for r in _sregs(ops[0]): val.pop(r, None)
            val.pop(ops[0], None)
            if v is not None: val[ops[0]] = v
            if ops[0] == "vcc": vcc, vcc_from_flag = v, False
        elif op == "s_cselect_b64" and scc is not None and _imm(ops[1]) is not None and _imm(ops[2]) is not None:
            val[ops[0]] = _imm(ops[1]) if scc else _imm(ops[2])
        elif op in ("s_andn2_b64", "s_and_b64") and ops[0] == "vcc" and ops[1] == "exec":
            f = val.get(ops[2])
            vcc = None if f is None else ((0 if f else 1) if op == "s_andn2_b64" else (1 if f else 0))      # exec is not empty
            vcc_from_flag = True
            scc = None if vcc is None else bool(vcc)
        elif op == "s_branch": nxt = K.label[ops[0]]; taken = True
        elif op.startswith("s_cbranch_"):
            c = op[10:]
            if c in ("scc0", "scc1"):
                if scc is None:
                    # the loop's own exit test (the trip count is not a class matter): the route ends at the latch
                    out.append((i, None)); return out, hops, "latch" if h in (i + 1, K.label[ops[0]]) else "scc unknown"
                taken = scc == (c == "scc1")
            elif c in ("vccz", "vccnz"):
                if vcc is None:
                    out.append((i, None)); return out, hops, "vcc unknown"
                taken = bool(vcc) == (c == "vccnz")
                if vcc_from_flag: hops.append(i)
            elif c == "execz": taken = False
            elif c == "execnz": taken = True
            else: raise AssertionError(op)
            if taken: nxt = K.label[ops[0]]
        elif op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_load", "s_buffer_load", "s_barrier", "s_endpgm", "s_setprio", "s_sleep")):
            # anything else that writes scalar registers: its destination is no longer known
            if ops:
                for r in _sregs(ops[0]): val.pop(r, None)
                val.pop(ops[0], None)
                if ops[0] in ("vcc", "vcc_lo", "vcc_hi"): vcc = None
            scc = None if op.startswith(("s_add", "s_sub", "s_and", "s_or", "s_xor", "s_lshl", "s_lshr", "s_ashr", "s_not", "s_andn2", "s_orn2", "s_bfe", "s_min", "s_max", "s_abs", "s_mul")) and not op.startswith("s_mul_") else scc
        elif op.startswith("v_cmp") and (not ops or ops[0] in ("vcc", "vcc_lo")): vcc = None; vcc_from_flag = False
        elif op.startswith("v_") and ops and _sregs(ops[0]):
            for r in _sregs(ops[0]): val.pop(r, None)
            val.pop(ops[0], None)
        out.append((i, taken))
        if op == "s_endpgm": return out, hops, "end"
        i = nxt
        if i == h: return out, hops, "latch"
    raise AssertionError("route does not end")


def count(K, seq):
    c = dict(salu=0, cbranch=0, cbranch_taken=0, branch=0, valu=0, smem=0, wait=0)
    for i, taken in seq:
        op = K.ins[i][1]
        if op == "s_branch": c["branch"] += 1
        elif op.startswith("s_cbranch_"):
            c["cbranch"] += 1; c["cbranch_taken"] += 1 if taken else 0
        elif op.startswith("s_waitcnt") or op == "s_nop": c["wait"] += 1
        elif op.startswith("s_load") or op.startswith("s_buffer_load"): c["smem"] += 1
        elif op.startswith("s_"): c["salu"] += 1
        elif op.startswith("v_"): c["valu"] += 1
    c["taken"] = c["cbranch_taken"] + c["branch"]
    return c


def route_table(K, header=None, classes=range(16)):
    """(header, classes: as for route; the pair loop's kinds are range(1, 7)) class -> counts of its static route from the loop header to the join (the first instruction all sixteen routes share behind
    the switch: the start of the accept chain), its flag-test hops on that stretch, and the unconditional branches between the end
    of the switch (the route's last s_cbranch_scc*) and the join"""
    classes = list(classes)
    h, at, _ = header or pass_header(K)
    routes = {}
    for c in classes:
        seq, hops, end = route(K, c, header)
        assert end == "latch" or seq, (c, end)
        routes[c] = (seq, hops, end)
    # the join: the routes are identical from it to the latch
    def suffix(a, b):
        n = 0
        while n < len(a) and n < len(b) and a[-1 - n][0] == b[-1 - n][0]: n += 1
        return n
    first = [i for i, _ in routes[classes[0]][0]]
    n = min(suffix(routes[classes[0]][0], routes[c][0]) for c in classes[1:])
    join = first[len(first) - n]
    table = {}
    for c in classes:
        seq, hops, end = routes[c]
        k = [i for i, _ in seq].index(join)
        head = seq[:k]
        t = count(K, head)
        last_scc = max([j for j, (i, _) in enumerate(head) if K.ins[i][1] in ("s_cbranch_scc0", "s_cbranch_scc1")], default=-1)
        behind = head[last_scc + 1:]
        t["flag_hops"] = len([i for i in hops if i in [x for x, _ in head]])
        t["branches_body_to_join"] = len([1 for i, _ in behind if K.ins[i][1] == "s_branch"])
        t["taken_body_to_join"] = len([1 for i, tk in behind if tk])
        t["labels"] = [l for i, _ in head for l, v in K.label.items() if v == i]
        t["end"] = end
        t["whole_iteration"] = count(K, seq)
        table[c] = t
    return table, K.ins[join][0]


# ---- the stretch between the pass and the shade block --------------------------------------------------------------------------
def shortest_route(K, start, goal):
    """the static route with the fewest instructions from instruction `start` to instruction `goal` (both included), every branch free
    to go either way - a lower bound of what a wave executes between the two: a list of instruction indices, None if there is none"""
    from collections import deque
    prev = {start: None}; todo = deque([start])
    while todo:
        i = todo.popleft()
        if i == goal: break
        succ = K.targets(i)[0]
        for t in succ:
            if t < len(K.ins) and t not in prev:
                prev[t] = i; todo.append(t)
    if goal not in prev: return None
    out = []; i = goal
    while i is not None: out.append(i); i = prev[i]
    return out[::-1]


def pass_exit(K):
    """index of the first instruction behind the record loop: where a wave stands when the pass's latch falls through"""
    ph = pass_header(K)[0]
    l = [x for x in loops(K) if x["header_index"] == ph]
    assert len(l) == 1 and len(l[0]["back_edges"]) == 1, l
    i = [k for k, ins in enumerate(K.ins) if ins[0] == l[0]["back_edges"][0]][0]
    assert K.ins[i][1].startswith("s_cbranch_scc"), K.ins[i]
    t = K.label[K.ins[i][2][0]]
    assert ph in (t, i + 1), K.ins[i]               # the latch branches back and falls out, or branches out and falls into the header
    return i + 1 if t == ph else t


def shade_start(K):
    """index of the shade block's first instruction: the path start's `depth < 0` compare, the nearest v_cmp_gt_i32 0 > v in front of the
    instruction that carries hash32's additive constant (the stream set-up of a new path, the first thing the block does)"""
    at = [k for k, ins in enumerate(K.ins) if "0xac564b05" in ins[2]]
    assert len(at) == 1, at
    for i in range(at[0], -1, -1):
        if K.ins[i][1].startswith("v_cmp_gt_i32") and "0" in K.ins[i][2]: return i
    raise AssertionError("no depth < 0 test in front of the path start")


def deal_route(K):
    """The stretch that produces nothing of the image: from the pass's latch through ONE deal of ONE round - the shortest static route
    that passes a read of lds_pixel_of_rank (ds_read_u8: only the deal has one; the masked regions it need not enter, such as the
    shadow ray's resolve behind the pass, are skipped in every kernel alike) - to the first instruction of the shade block.
    Returns (instruction indices, counts): VALU, scalar ALU, LDS reads, and the s_waitcnt that wait for lgkmcnt."""
    a, b = pass_exit(K), shade_start(K)
    best = None
    for w in [k for k, ins in enumerate(K.ins) if ins[1] == "ds_read_u8"]:
        r1, r2 = shortest_route(K, a, w), shortest_route(K, w, b)
        if r1 is None or r2 is None: continue
        r = r1 + r2[1:-1]                    # (the shade block's first instruction is where the route ends, not part of it)
        if best is None or len(r) < len(best): best = r
    assert best, "no route from the pass through a deal to the shade block in " + K.name
    c = dict(valu=0, salu=0, lds=0, smem=0, lgkm_waits=0, instructions=len(best))
    for i in best:
        op, ops = K.ins[i][1], K.ins[i][2]
        if op.startswith("v_"): c["valu"] += 1
        elif op.startswith("ds_"): c["lds"] += 1
        elif op.startswith("s_load") or op.startswith("s_buffer_load"): c["smem"] += 1
        elif op.startswith("s_waitcnt"): c["lgkm_waits"] += 1 if any("lgkmcnt" in o for o in ops) else 0
        elif op.startswith("s_") and op != "s_nop": c["salu"] += 1
    return best, c


# ---- control-flow integrity ---------------------------------------------------------------------------------------------------
def check_exec_regions(K):
    """Every s_and_saveexec_b64 sD, ... must be closed by s_or_b64 exec, exec, sD on every route from it to a loop latch or the kernel's
    end, with sD not written in between.  Walks all static routes from each open (each instruction once per open): returns a list of
    violations, [] when every open is closed on every route.  (An s_andn2_b64 exec, exec, x / s_and_b64 exec, ... that narrows exec
    inside a loop is the other idiom, loop-carried masks; it is reported in `narrowing` for reading, not judged.)"""
    bad = []; opens = []; narrowing = []
    for i, (line, op, ops) in enumerate(K.ins):
        if op in ("s_and_saveexec_b64", "s_or_saveexec_b64", "s_andn2_saveexec_b64"): opens.append(i)
        elif op.startswith("s_") and ops and ops[0] == "exec" and not (op == "s_or_b64"): narrowing.append(line)
    # The backend's idioms (SILowerControlFlow): if = s_and_saveexec_b64 T, cond [; s_xor_b64 M, exec, T: the lanes left out] ...
    # s_or_b64 exec, exec, M; else = s_andn2_saveexec_b64 M2, M (or s_or_saveexec_b64 M2, M ; s_xor_b64 exec, exec, M2) ... s_or_b64
    # exec, exec, M2.  So the register that holds "the lanes to give back" moves: it is followed through these forms.
    for o in opens:
        if K.ins[o][1] != "s_and_saveexec_b64": continue           # (an else arm: followed from its if)
        seen = set(); todo = [(o + 1, K.ins[o][2][0])]; closed = 0
        while todo:
            i, mask = todo.pop()
            if (i, mask) in seen: continue
            seen.add((i, mask))
            if i == o:
                bad.append((K.ins[o][0], "reached again before its close")); continue
            line, op, ops = K.ins[i]
            if op == "s_or_b64" and ops[0] == "exec" and mask in ops[1:]:
                closed += 1; continue
            if op == "s_endpgm":
                bad.append((K.ins[o][0], "kernel end at line %d with the region open" % line)); continue
            if op == "s_xor_b64" and ops[1] == "exec" and ops[2] == mask and ops[0] != "exec": mask = ops[0]
            elif op in ("s_andn2_saveexec_b64", "s_or_saveexec_b64") and ops[1] == mask: mask = ops[0]
            elif op == "s_xor_b64" and ops[0] == "exec" and mask in ops[1:]: pass
            elif ops and op.startswith(("s_", "v_cmp", "v_readlane", "v_readfirstlane", "v_mad_u64", "v_add_co", "v_sub_co")) and set(_sregs(ops[0]) + (_sregs(ops[1]) if op.startswith(("v_mad_u64", "v_add_co", "v_sub_co")) and len(ops) > 1 else [])) & set(_sregs(mask)) \
                    and not op.startswith(("s_cmp", "s_cbranch", "s_branch", "s_bitcmp", "s_waitcnt")):
                bad.append((K.ins[o][0], "mask %s written at line %d (%s) before the close" % (mask, line, op))); continue
            todo.extend((t, mask) for t in K.targets(i)[0])
        if closed == 0: bad.append((K.ins[o][0], "never closed"))
    return bad, len(opens), narrowing


def loops(K):
    """Natural loops of the kernel's control-flow graph: [{header: source line, depth, back_edges: [source line of the latch's last
    instruction], exits: number of edges that leave the loop, size: instructions}], outermost first.  A back edge is an edge whose
    target dominates its source (dominators by the iterative algorithm over basic blocks)."""
    n = len(K.ins)
    leaders = {0} | set(K.label.values())
    for i in range(n):
        succ, kind = K.targets(i)
        if kind: leaders.update(s for s in succ if s < n); leaders.add(i + 1)
    leaders = sorted(l for l in leaders if l < n)
    start_of = {}
    for b, l in enumerate(leaders):
        for i in range(l, leaders[b + 1] if b + 1 < len(leaders) else n): start_of[i] = b
    succs = []
    for b, l in enumerate(leaders):
        last = (leaders[b + 1] if b + 1 < len(leaders) else n) - 1
        succs.append(sorted(set(start_of[s] for s in K.targets(last)[0] if s < n)))
    preds = [[] for _ in leaders]
    for b, ss in enumerate(succs):
        for s in ss: preds[s].append(b)
    # reverse post-order from the entry
    order = []; seen = set(); stack = [(0, iter(succs[0]))]; seen.add(0)
    while stack:
        b, it = stack[-1]
        for s in it:
            if s not in seen:
                seen.add(s); stack.append((s, iter(succs[s]))); break
        else:
            order.append(b); stack.pop()
    order.reverse()
    full = set(order)
    dom = {b: set(full) for b in order}; dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for b in order[1:]:
            ps = [dom[p] for p in preds[b] if p in full]
            new = set.intersection(*ps) | {b} if ps else {b}
            if new != dom[b]: dom[b] = new; changed = True
    found = {}
    for b in order:
        for s in succs[b]:
            if s in dom[b]: found.setdefault(s, []).append(b)
    out = []
    for h, latches in found.items():
        body = {h}; todo = list(latches)
        while todo:
            x = todo.pop()
            if x in body: continue
            body.add(x); todo.extend(p for p in preds[x] if p in full)
        end = lambda b: (leaders[b + 1] if b + 1 < len(leaders) else n) - 1
        out.append(dict(header=K.ins[leaders[h]][0], header_index=leaders[h], body=body, back_edges=sorted(K.ins[end(b)][0] for b in latches),
                        exits=sum(1 for b in body for s in succs[b] if s not in body), size=sum(end(b) - leaders[b] + 1 for b in body)))
    for l in out: l["depth"] = sum(1 for m in out if l["body"] < m["body"]) + 1
    out.sort(key=lambda l: (l["depth"], l["header"]))
    for l in out: l["blocks"] = len(l.pop("body"))
    return out


def main():
    if sys.argv[1] == "--routes":
        K = Kernel(sys.argv[2], sys.argv[3])
        table, join_line = route_table(K)
        print("%s\njoin (accept chain) at line %d; metadata %s" % (K.name, join_line, K.meta))
        keys = ("salu", "cbranch", "cbranch_taken", "branch", "taken", "flag_hops", "branches_body_to_join", "valu")
        print("class " + " ".join("%8s" % k[:8] for k in keys))
        for c in range(16): print("%5d " % c + " ".join("%8d" % table[c][k] for k in keys) + "   " + " ".join(table[c]["labels"]))
        if len(sys.argv) > 4:
            cl = [int(x) for x in sys.argv[4].split(",")]
            print("sum over " + str(cl) + ": " + str({k: sum(table[c][k] for c in cl) for k in keys}))
            print("whole iterations: " + str({k: sum(table[c]["whole_iteration"][k] for c in cl) for k in ("salu", "cbranch", "cbranch_taken", "branch", "taken", "valu", "smem", "wait")}))
        bad, n, narrowing = check_exec_regions(K)
        print("saveexec regions: %d, violations: %s; other writes of exec at lines %s" % (n, bad, narrowing))
        try: print("pass latch -> one deal of one round -> shade block: %s" % deal_route(K)[1])
        except AssertionError as e: print("no deal route: %s" % e)
        ph = pass_header(K)[0]
        pp = pair_header(K)[0] if len(nibble_headers(K)) == 2 else -1
        if pp >= 0:
            # the pair unit: the pair loop's six kinds, header to join (both records' arithmetic) and the whole turn (with the accept)
            ptable, pjoin = route_table(K, pair_header(K), range(1, 7))
            print("pair loop: join (shared accept) at line %d" % pjoin)
            print(" kind " + " ".join("%8s" % k[:8] for k in keys) + "    whole turn: valu salu smem")
            for c in range(1, 7):
                w = ptable[c]["whole_iteration"]
                print("%5d " % c + " ".join("%8d" % ptable[c][k] for k in keys) + "   %22d %4d %4d" % (w["valu"], w["salu"] + w["cbranch"] + w["branch"], w["smem"]))
        for l in loops(K):
            print("loop: depth %d header line %5d%s: %d back edge(s) from %s, %d exit edge(s), %d instructions" %
                  (l["depth"], l["header"], " (the pass)" if l["header_index"] == ph else " (the pair loop)" if l["header_index"] == pp else "", len(l["back_edges"]), l["back_edges"], l["exits"], l["size"]))
        return
    path = sys.argv[1]; want = sys.argv[2] if len(sys.argv) > 2 else None
    blocks = blocks_of(path, want)
    tot = dict(valu=0, salu=0, vmem=0, lds=0)
    for b in blocks:
        for k in tot: tot[k] += b[k]
        print(f"{b['label']:14s} L{b['line']:6d} valu {b['valu']:4d} (half {b['half']:3d} trans {b['trans']:2d}) salu {b['salu']:3d} vmem {b['vmem']:2d} lds {b['lds']:2d} smem {b['smem']:2d} wait {b['wait']:2d}  {' '.join(b['br'])}")
    print("total", tot)


if __name__ == "__main__":
    main()
