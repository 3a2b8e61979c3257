"""Build-time check of the generated code of conv_xk.hip (csrc/Makefile, run by __graft_entry__.build(); the kernel names of its two
predecessors, conv_xp / conv_xw, are still understood: the unit test feeds synthetic listings under them).

The kernel issues its matrix instructions as asm statements, so hipcc inserts none of the wait states an accumulator access needs
(MI355X: no hardware interlock between a matrix write and a vector read of the same register).  The sources are structured so that
hipcc never has a reason to touch an accumulator; this script proves it on the ISA of every instantiation:
  * the matrix instructions use exactly the expected accumulator tuples (conv_xp: 2 NT, conv_xw: 4 NT, conv_xk: MT NT - MT, the M tiles of
    a tile, is the kernel's second template argument; the three-argument name of before means 4), the same registers throughout;
  * no v_accvgpr_mov / v_accvgpr_write (or any other non-matrix instruction) writes an accumulator register;
  * every read of an accumulator register sits behind the epilogue's tied wait (s_nop 15) IN THE SAME BASIC BLOCK with no matrix
    instruction in between: the "behind the wait" state is dropped at every label and after every branch, so a read reached through a
    back edge or a branch target from a block that ends in a matrix instruction cannot pass (round-4 advisor finding).
A conv_xk kernel for layers with a half-height bottom tile row holds TWO walks behind one wave-uniform branch at its entry, MT = 4 and
MT = 2; the source marks the start of each with an asm comment "; conv_xk walk MT = <n>".  Every walk is checked as a body of its own,
against its own MT NT tuples (a register that is an accumulator in one walk may hold an operand fragment in the other); what stands
in front of the first mark must not hold a matrix instruction.  Without marks the kernel is one body of the name's MT.
conv_xw keeps two operand fragment sets (64 registers) in the accumulator half of the register file as well: those are written by LDS
reads and read by matrix instructions only, and are not accumulators.
usage: check_xp_isa.py conv_xk.s | conv_xk.tune.s"""
import re
import sys


def regs(tok):
    m = re.fullmatch(r'a\[(\d+):(\d+)\]', tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r'a(\d+)', tok)
    return {int(m.group(1))} if m else set()


WALK = re.compile(r'; conv_xk walk MT = (\d)')


def check(name, lines):
    """-> (NT, accumulator tuples of all bodies, errors) of one kernel's listing (instructions, labels and walk marks)"""
    m = re.search(r'conv_x([pwk])_kernelILi(\d)E(?:Li(\d)E)?', name)
    nt = int(m.group(2))
    per_nt = 2 if m.group(1) == 'p' else int(m.group(3) or 4)
    bodies, marked = [(per_nt, [])], False
    for ln in lines:
        w = WALK.match(ln)
        if w:
            if not marked:
                bodies, marked = [(0, bodies[0][1])], True      # the kernel's entry: nothing of the matrix pipe
            bodies.append((int(w.group(1)), []))
        else:
            bodies[-1][1].append(ln)
    ntup, errs = 0, []
    for mt, body in bodies:
        n, e = check_body(mt * nt, body)
        ntup += n
        errs += ['MT = %d walk: %s' % (mt, x) for x in e] if marked else e
    return nt, ntup, errs


def check_body(expected, lines):
    acc, tuples = set(), set()
    for ln in lines:
        if ln.startswith('v_mfma'):
            dst = ln.split()[1].rstrip(',')
            tuples.add(dst)
            acc |= regs(dst)
    errs = []
    if len(tuples) != expected or len(acc) != 16 * expected:
        errs.append('%d accumulator tuples (%d registers), expected %d (%d)' % (len(tuples), len(acc), expected, 16 * expected))
    behind_tie = False
    for i, ln in enumerate(lines):
        if ln.endswith(':') or ln.startswith(('s_cbranch', 's_branch', 's_setpc', 's_endpgm')):
            behind_tie = False                       # a basic-block boundary: whatever protected the reads above does not reach across
            continue
        if ln.startswith('v_mfma'):
            behind_tie = False
            continue
        if ln.startswith('s_nop 15'):
            behind_tie = True
            continue
        toks = [t.rstrip(',') for t in ln.split()[1:]]
        touched = [t for t in toks if regs(t) & acc]
        if not touched:
            continue
        writes = bool(toks) and bool(regs(toks[0]) & acc) and not ln.startswith(('buffer_store', 'global_store', 'ds_write', 'scratch_store'))
        if writes:
            errs.append('line %d writes an accumulator: %s' % (i, ln))
        elif not behind_tie:
            errs.append('line %d reads an accumulator in the shadow of a matrix instruction: %s' % (i, ln))
    return len(tuples), errs


def main(path):
    text = open(path).read().split('\n')
    kernels, cur, name = {}, None, None
    for ln in text:
        m = re.match(r'^(_ZN3csd14conv_x[pwk]_kernel\w+):', ln)
        if m:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            t = ln.strip()
            if t.startswith('s_endpgm'):
                kernels[name] = cur
                cur = None
            elif WALK.match(t):
                cur.append(t)
            elif t and not t.startswith(';') and (not t.startswith('.') or t.split(';')[0].strip().endswith(':')):
                # directives (.p2align, .loc ...) are dropped; LABELS (.LBB0_3:) are kept - they are the basic-block boundaries check()
                # drops its "behind the wait" state at (round-5 advisor finding: they used to be filtered with the directives)
                cur.append(t.split(';')[0].strip())
    if not kernels:
        print('check_xp_isa: no conv_xk kernel in', path)
        return 1
    bad = 0
    for name, lines in sorted(kernels.items()):
        nt, ntup, errs = check(name, lines)
        print('%s: NT = %d, %d accumulator tuples, %d instructions: %s' % (name, nt, ntup, len(lines), 'ok' if not errs else 'FAILED'))
        for e in errs[:10]:
            print('   ', e)
        bad += bool(errs)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1]))
