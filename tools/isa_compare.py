#!/usr/bin/env python3
"""Machine-code comparison of two builds of libsatmi.so, kernel by kernel (no GPU).

    python tools/isa_compare.py PARENT_LIB [NEW_LIB]

For every kernel descriptor (*.kd) of either library: satmi.isa.kernel_code_sha of
the kernel's symbols in both, and whether they agree.  Exit status 1 when a
kernel of PARENT_LIB is missing from NEW_LIB or hashes differently; kernels that
only NEW_LIB has are listed as new."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sat-mpi-stana-andrei_amd"))

from satmi import _capi, isa  # noqa: E402


def kernels(path):
    with open(path, "rb") as fh:
        data = fh.read()
    return sorted({name[:-3] for co in isa.code_objects(data) for name, _ in isa.elf_symbols(co)
                   if name.endswith(".kd")})


def main():
    parent = sys.argv[1]
    new = sys.argv[2] if len(sys.argv) > 2 else _capi.LIB_PATH
    kp, kn = kernels(parent), kernels(new)
    bad = 0
    print(f"# parent: {len(kp)} kernel descriptors; new: {len(kn)}")
    for k in sorted(set(kp) | set(kn)):
        a = isa.kernel_code_sha(k, parent) if k in kp else None
        b = isa.kernel_code_sha(k, new) if k in kn else None
        verdict = "new" if a is None else "MISSING" if b is None else "same" if a == b else "DIFFERENT"
        bad += verdict in ("MISSING", "DIFFERENT")
        print(f"{verdict:9s} {a or '-':16s} {b or '-':16s} {k}")
    print(f"# {len(kp) - bad} of the parent's {len(kp)} kernels are byte-identical in the new library, {bad} are not")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
