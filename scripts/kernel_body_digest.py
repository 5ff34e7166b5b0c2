#!/usr/bin/env python3
"""sha256 of ONE kernel's instructions in a device listing of scripts/device_listing.sh: the gate for a change that adds a kernel to a
translation unit (the unit's own digest then moves) and must leave the kernels already there as they are.
  scripts/kernel_body_digest.py LISTING.s [NAME_PART ...]
Prints one line per kernel of the listing whose symbol contains every NAME_PART: digest, instruction lines, symbol.  The body is the
text between the kernel's label and the section of its kernel descriptor, without comments, with the kernel's own symbol and the
function number of its block labels (.LBB<n>_<m>: the kernel's position in the unit) blanked - what remains is the instruction
stream with its operands and branch targets.  Two trees compile a kernel to the same code exactly when these lines agree; the
descriptor (kernarg size, register counts) is not part of it: compare .vgpr_count / .sgpr_spill_count in the listing's metadata."""
import hashlib
import re
import sys


def kernels(text):
    lines = text.split('\n')
    for i, line in enumerate(lines):
        m = re.match(r'^(\w+):\s+; @\1\s*$', line)
        if not m:
            continue
        sym = m.group(1)
        end = next((k for k in range(i, len(lines)) if lines[k].lstrip().startswith(('.section', '.Lfunc_end'))), len(lines))      # (a truncated listing: to its end)
        body = []
        for b in lines[i + 1:end]:
            b = b.split(';')[0].rstrip().replace(sym, 'KERNEL')
            b = re.sub(r'\.LBB\d+_', '.LBB_', b)
            if b.strip():
                body.append(b)
        yield sym, body


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    with open(argv[1]) as f:
        text = f.read()
    for sym, body in kernels(text):
        if all(p in sym for p in argv[2:]):
            print(hashlib.sha256('\n'.join(body).encode()).hexdigest(), len(body), sym)


if __name__ == '__main__':
    main(sys.argv)
