#!/usr/bin/env python3
"""Build container: compare two device-assembly listings of one csrc file kernel by kernel (no GPU needed).

    cd illuminant_amd/csrc
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -fno-slp-vectorize --cuda-device-only -S particles.hip -o new.s
    (the same in a checkout of the other commit -> base.s)
    tools/isa_compare.py base.s new.s

Per kernel: SAME when the instruction streams are equal once branch labels are normalised, else diff; then the counts of vector (v_*),
scalar (s_*) and memory / other instructions, VGPRs, scratch and occupancy, each as base->new.  Complements tools/kernel_resources.sh,
which reports what the compiler allocates but not whether the code moved.
"""
import hashlib
import re
import subprocess
import sys


def parse(path):
    kernels, cur = {}, None
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        if m:
            cur = kernels.setdefault(m.group(1), {'v': 0, 's': 0, 'm': 0, 'hash': hashlib.md5(), 'body': True})
            continue
        if cur is None:
            continue
        t = line.strip()
        m = re.match(r';\s*(NumVgprs|ScratchSize|Occupancy):\s*(\d+)', t)     # the metadata follows the body
        if m:
            cur.setdefault(m.group(1), m.group(2))
            continue
        if line.startswith('.Lfunc_end'):
            cur['body'] = False
        if not cur['body'] or not t or t.startswith(('.', ';', '//')) or t.endswith(':'):
            continue
        op = t.split()[0]
        cur['v' if op.startswith('v_') else 's' if op.startswith('s_') else 'm'] += 1
        cur['hash'].update(re.sub(r'\.LBB\d+_\d+', 'L', t.split(';')[0]).encode())
    return kernels


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    print('only in base:', sorted(set(a) - set(b)) or 'none', '| only in new:', sorted(set(b) - set(a)) or 'none')
    names = subprocess.run(['c++filt'], input='\n'.join(a), capture_output=True, text=True).stdout.splitlines()
    same = 0
    for k, n in zip(a, names):
        if k not in b:
            continue
        x, y = a[k], b[k]
        equal = x['hash'].hexdigest() == y['hash'].hexdigest()
        same += equal
        n = re.sub(r'\(.*', '', n).replace('void ', '').replace('ilm::', '')
        print('%-58s %s v %d->%d s %d->%d m %d->%d | vgpr %s->%s scratch %s->%s occ %s->%s' % (
            n[:58], 'SAME' if equal else 'diff', x['v'], y['v'], x['s'], y['s'], x['m'], y['m'], x.get('NumVgprs'), y.get('NumVgprs'),
            x.get('ScratchSize'), y.get('ScratchSize'), x.get('Occupancy'), y.get('Occupancy')))
    print('%d of %d kernels have identical instruction streams' % (same, len(set(a) & set(b))))


if __name__ == '__main__':
    main()
