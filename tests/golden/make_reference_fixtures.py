"""Records what the tests check against the reference as data fixtures, so that the suite needs no reference checkout.

    python tests/golden/make_reference_fixtures.py <reference checkout>

writes
  tests/golden/data/*.yaml     the reference's model inputs (data/*.yaml, copied byte for byte)
  tests/golden/reference.json  facts read from the reference's build files:
                                 make_check_states / make_check_matvec  the file lists of `make check` (Makefile:88-125)
                                 primme_params                          offsets of n, nLocal, matrix in PRIMME 3.1's
                                                                        primme_params (x86-64, 64-bit PRIMME_INT), from
                                                                        compiling offsetof() against its primme_headers/
Nothing here is reference *source*; these are inputs and the numbers read from it.
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def make_check_lists(ref):
    with open(os.path.join(ref, "Makefile"), encoding="utf-8") as f:
        mk = f.read()
    states = re.findall(r"--kRepresentatives data/matvec/(\w+)\.h5", mk.split("check-states-enumeration:")[1].split(".PHONY")[0])
    matvec = re.findall(r"--kVectors data/matvec/(\w+)\.h5", mk.split("check-matrix-vector-product:")[1].split("TEST_DATA_URL")[0])
    return states, matvec


def primme_offsets(ref):
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "off.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "primme.h"\n'
                    'int main(void){printf("%zu %zu %zu\\n", offsetof(primme_params,n), offsetof(primme_params,nLocal),'
                    ' offsetof(primme_params,matrix));return 0;}\n')
        exe = os.path.join(d, "off")
        subprocess.check_call(["gcc", "-I", os.path.join(ref, "primme_headers"), src, "-o", exe])
        n, n_local, matrix = (int(t) for t in subprocess.check_output([exe]).split())
    return {"n": n, "nLocal": n_local, "matrix": matrix}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    data = os.path.join(HERE, "data")
    os.makedirs(data, exist_ok=True)
    src = os.path.join(ref, "data")
    for name in sorted(os.listdir(src)):
        if name.endswith(".yaml"):
            shutil.copyfile(os.path.join(src, name), os.path.join(data, name))
    states, matvec = make_check_lists(ref)
    facts = {"make_check_states": states, "make_check_matvec": matvec,
             "primme_params": {"version": "3.1", "abi": "x86-64, 64-bit PRIMME_INT", "offsetof": primme_offsets(ref)}}
    with open(os.path.join(HERE, "reference.json"), "w", encoding="utf-8") as f:
        json.dump(facts, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
