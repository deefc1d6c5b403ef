"""Print registers / spills / LDS of every kernel in an AMDGPU assembly file (hipcc -save-temps): tools/kernel_regs.py file.s [filter]

Per kernel also how often it moves a scalar to or from a VGPR lane (v_writelane_b32 / v_readlane_b32: the SGPR spills, which the
metadata does not count), in the whole kernel and inside its longest loop (the span of the backward branch that covers the most
instructions: step_kernel's per-second loop)."""
import re
import sys


def lane_moves(asm, name):
    """-> (v_readlane, v_writelane in the kernel, instructions, v_readlane, v_writelane in its longest loop)"""
    try:
        body = asm[asm.index('\n%s:' % name) + 1:asm.index('.amdhsa_kernel %s\n' % name)]
    except ValueError:
        return None
    ins, labels = [], {}
    for ln in body.split('\n'):
        ln = re.sub(r'\s*;.*$', '', ln).strip()
        if ln.endswith(':'):
            labels[ln[:-1]] = len(ins)
        elif ln and not ln.startswith('.'):
            ins.append(ln)
    lo = hi = 0
    for i, s in enumerate(ins):
        m = re.match(r's_c?branch\S*\s+(\S+)', s)
        if m and labels.get(m[1], i + 1) <= i and i - labels[m[1]] > hi - lo:
            lo, hi = labels[m[1]], i
    n = lambda op, a, b: sum(1 for s in ins[a:b] if s.startswith(op))
    return (n('v_readlane_b32', 0, len(ins)), n('v_writelane_b32', 0, len(ins)), hi + 1 - lo if hi else 0,
            n('v_readlane_b32', lo, hi + 1), n('v_writelane_b32', lo, hi + 1))


txt = open(sys.argv[1]).read()
flt = sys.argv[2] if len(sys.argv) > 2 else ''
for blk in txt.split('  - .agpr_count:')[1:]:
    get = lambda k: (re.search(r'\.%s:\s+(\S+)' % k, blk) or [None, '?'])[1]
    name = get('name')
    if flt in name:
        mv = lane_moves(txt, name)
        print('%-90s vgpr %s agpr %s sgpr %s spill %s scratch %s lds %s' % (name[:90], get('vgpr_count'), blk.split()[0], get('sgpr_count'),
                                                                         get('vgpr_spill_count'), get('private_segment_fixed_size'),
                                                                         get('group_segment_fixed_size'))
              + ('' if mv is None else ' readlane %d writelane %d loop %d (readlane %d writelane %d)' % mv))
