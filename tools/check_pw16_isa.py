"""Build-time check of the generated code of conv_pw16.hip (csrc/Makefile, run by __graft_entry__.build()).

pw16_kernel addresses its output and its residual through buffer descriptors.  A descriptor hipcc cannot prove wave-uniform (one built
from threadIdx.x >> 6, say) is not rejected: every access through it is wrapped in a "waterfall" loop - v_readfirstlane of the four
descriptor words, a compare, s_and_saveexec, the access, s_xor exec, s_cbranch_execnz back - which runs once, costs a dozen
instructions per access and keeps the accesses from overlapping.  The same shape appears around any memory access inside a loop whose
trip count differs between lanes.  This script fails the build if, in any pw16_kernel instantiation, a loop closed by s_cbranch_execnz
(a backward branch to a label) contains a buffer_ or global_ instruction.
usage: check_pw16_isa.py conv_pw16.s"""
import re
import sys


def blocks_of(lines):
    """basic blocks of one kernel: (list of [first, last + 1) line ranges, label -> block, successor lists)"""
    starts = {0}
    for i, ln in enumerate(lines):
        if ln.endswith(':'):
            starts.add(i)
        elif ln.startswith(('s_cbranch', 's_branch', 's_setpc', 's_endpgm')):
            starts.add(i + 1)
    cuts = sorted(s for s in starts if s < len(lines)) + [len(lines)]
    spans = list(zip(cuts[:-1], cuts[1:]))
    label_block = {lines[a][:-1]: b for b, (a, _) in enumerate(spans) if lines[a].endswith(':')}
    succ = []
    for b, (a, e) in enumerate(spans):
        last = lines[e - 1]
        out = []
        m = re.match(r's_c?branch\w*\s+(\S+)', last)
        if m and m.group(1) in label_block:
            out.append(label_block[m.group(1)])
        if not last.startswith(('s_branch', 's_setpc', 's_endpgm')) and b + 1 < len(spans):
            out.append(b + 1)
        succ.append(out)
    return spans, label_block, succ


def reach(start, succ):
    seen, todo = {start}, [start]
    while todo:
        for n in succ[todo.pop()]:
            if n not in seen:
                seen.add(n)
                todo.append(n)
    return seen


def dominators(succ):
    """block -> set of the blocks every path from block 0 to it passes through"""
    n = len(succ)
    pred = [[] for _ in range(n)]
    for b, out in enumerate(succ):
        for t in out:
            pred[t].append(b)
    live = reach(0, succ)
    dom = [set(live) for _ in range(n)]
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for b in sorted(live - {0}):
            ps = [dom[p] for p in pred[b] if p in live]
            new = (set.intersection(*ps) if ps else set()) | {b}
            if new != dom[b]:
                dom[b], changed = new, True
    return dom, pred


def check(lines):
    """lines: instructions and labels of one kernel -> list of error strings.  A loop closed by s_cbranch_execnz: the branch's target
    dominates the branch (a back edge; an out-of-line block that rejoins earlier code is none); its body: the blocks that reach the
    branch without passing through the target."""
    spans, label_block, succ = blocks_of(lines)
    dom, pred = dominators(succ)
    errs = []
    for b, (a, e) in enumerate(spans):
        m = re.match(r's_cbranch_execnz\s+(\S+)', lines[e - 1])
        if not m or m.group(1) not in label_block:
            continue
        head = label_block[m.group(1)]
        if head not in dom[b]:
            continue
        body, todo = {head, b}, [b] if b != head else []
        while todo:
            for p in pred[todo.pop()]:
                if p not in body:
                    body.add(p)
                    todo.append(p)
        mem = [ln for blk in sorted(body) for ln in lines[spans[blk][0]:spans[blk][1]] if ln.startswith(('buffer_', 'global_'))]
        if mem:
            errs.append('loop %s .. line %d (s_cbranch_execnz) contains %d memory accesses, first: %s' % (m.group(1), e - 1, len(mem), mem[0]))
    return errs


def main(path):
    text = open(path).read().split('\n')
    kernels, cur, name = {}, None, None
    for ln in text:
        m = re.match(r'^(_ZN3csd11pw16_kernel\w+):', ln)
        if m:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            t = ln.split(';')[0].strip()
            if t.startswith('s_endpgm'):
                kernels[name] = cur
                cur = None
            elif t and (not t.startswith('.') or t.endswith(':')):       # directives are dropped, labels (.LBB0_3:) kept
                cur.append(t)
    if not kernels:
        print('check_pw16_isa: no pw16_kernel in', path)
        return 1
    bad = 0
    for name, lines in sorted(kernels.items()):
        errs = check(lines)
        print('%s: %d instructions: %s' % (name, sum(not l.endswith(':') for l in lines), 'ok' if not errs else 'FAILED'))
        for e in errs[:10]:
            print('   ', e)
        bad += bool(errs)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1]))
