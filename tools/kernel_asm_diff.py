#!/usr/bin/env python
"""Compare the kernels of two builds by their device assembly (hipcc -save-temps=obj ... *gfx950*.s), across translation units.

    python tools/kernel_asm_diff.py DIR_A DIR_B

Every *gfx950*.s of a directory is split into kernels at the `<mangled name>:` ... `.Lfunc_endN:` pairs; `;` comments go and
`.LBB<n>_` becomes `.LBB_` (block labels carry the function's index in its file, so a whole-file diff cannot work once a kernel
has moved to another file).  Reports kernels missing, extra, duplicated or different in text, and any difference in the
isa_meta.kernels fields (VGPRs, AGPRs, scratch, spills, LDS).  Exit status 0 = identical.
"""
import glob
import os
import re
import sys

import isa_meta

FIELDS = ('vgpr', 'agpr', 'vgpr_spill', 'sgpr_spill', 'scratch', 'loop_scratch', 'lds')


def load(d):
    text, meta, dup = {}, {}, []
    for path in sorted(glob.glob(os.path.join(d, '*gfx950*.s'))):
        ks = {k['mangled']: k for k in isa_meta.kernels(path)}
        cur = None
        for line in open(path):
            line = re.sub(r'\.LBB\d+_', '.LBB_', line.split(';')[0]).rstrip()
            if cur is None and line[:-1] in ks and line.endswith(':'):
                cur = line[:-1]
                if cur in text:
                    dup.append(cur)
                text[cur], meta[cur] = [], ks[cur]
            elif cur is not None and line.startswith('.Lfunc_end'):
                cur = None
            elif cur is not None and line:
                text[cur].append(line)
    return text, meta, dup


if __name__ == '__main__':
    (ta, ma, da), (tb, mb, db) = load(sys.argv[1]), load(sys.argv[2])
    both = sorted(set(ta) & set(tb))
    rep = {'missing': sorted(set(ta) - set(tb)), 'extra': sorted(set(tb) - set(ta)), 'duplicated': da + db,
           'different instructions': [n for n in both if ta[n] != tb[n]],
           'different metadata': [n for n in both if any(ma[n][f] != mb[n][f] for f in FIELDS)]}
    print('%d kernels in %s, %d in %s' % (len(ta), sys.argv[1], len(tb), sys.argv[2]))
    for what, names in rep.items():
        print('%s: %d' % (what, len(names)))
        for n in names:
            print('   ', ma.get(n, mb.get(n))['name'], n)
    sys.exit(1 if any(rep.values()) else 0)
