"""Which kernels of two builds of one source differ in machine code: tools/isa_diff.py OLD NEW [old_name=new_name ...]

OLD / NEW are two .hip sources (each where its #includes resolve; compiled to device-only gfx950 assembly with build.FLAGS) or two .s
files.  A kernel is the text from its label through .end_amdhsa_kernel -- instructions and kernel descriptor (registers, scratch, LDS) --
without comments, with label numbers and its own symbol blanked.  Kernels pair by symbol; a renamed one by old_name=new_name, each side
a piece of the (mangled) symbol that only that kernel has, e.g. head_bwd2_kernel=head_bwd_kernelITpTnbJEEE.  Exit status 1 if anything
differs.  Host only; this is the comparison behind the comments that say "measured by comparing the assembly"."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from deeprl_signal_control_amd.build import FLAGS, HIPCC


def assembly(path):
    if path.endswith('.s'):
        return open(path).read()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'out.s')
        subprocess.check_call([HIPCC] + [f for f in FLAGS if f != '-shared'] + ['--cuda-device-only', '-S', path, '-o', out])
        return open(out).read()


def kernels(asm):
    """-> {symbol: (normalised lines, 'vgpr .. sgpr .. scratch ..' of the kernel's metadata)}"""
    out = {}
    for sym in re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', asm, re.M):
        body = asm[asm.index('\n%s:' % sym) + 1:asm.index('.end_amdhsa_kernel', asm.index('.amdhsa_kernel %s\n' % sym))]
        lines = [re.sub(r'\.L([A-Za-z_]+)\d+', r'.L\1', re.sub(r'\s*;.*$', '', ln).replace(sym, 'KERNEL')).strip() for ln in body.split('\n')]
        meta = asm[asm.index('.name:', asm.index('amdhsa.kernels:')):]
        meta = meta[meta.index('.name:           %s\n' % sym):]
        regs = ' '.join('%s %s' % (k, re.search(r'\.%s:\s+(\S+)' % f, meta)[1]) for k, f in
                        (('scratch', 'private_segment_fixed_size'), ('sgpr', 'sgpr_count'), ('vgpr', 'vgpr_count')))
        out[sym] = ([ln for ln in lines if ln], regs)
    return out


def main(old, new, *pairs):
    a, b = kernels(assembly(old)), kernels(assembly(new))
    for p in pairs:
        (ka,), (kb,) = ([k for k in d if s in k] for d, s in zip((a, b), p.split('=')))
        print('paired  %s = %s: %d lines, %s | %d lines, %s' % (*p.split('='), len(a[ka][0]), a[ka][1], len(b[kb][0]), b[kb][1]))
        a[kb] = a.pop(ka)
    diff = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
    for k in diff:
        print('DIFFERS %s: %d lines, %s | %d lines, %s' % (k, len(a[k][0]), a[k][1], len(b[k][0]), b[k][1]))
    for tag, ks in (('only in OLD', a.keys() - b.keys()), ('only in NEW', b.keys() - a.keys())):
        for k in sorted(ks):
            print('%s %s' % (tag, k))
    print('%d kernels in OLD, %d in NEW, %d in both, %d of them differ' % (len(a), len(b), len(a.keys() & b.keys()), len(diff)))
    return 1 if diff or a.keys() != b.keys() else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:]))
