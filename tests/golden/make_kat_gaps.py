"""Generates tests/golden/spoa_kat_gaps.json: spoa's 18 alignment known-answer tests (Local*, Global*, SemiGlobal* of
vendor/spoa/test/spoa_test.cpp), read as data -- for each, the alignment type, the six scores of its Setup(...) line, the
quality flag and the consensus string it asserts.  Linear, affine and convex gaps; the reads are tests/golden/sample.fastq.gz
(spoa's own test data).  Nothing but these values is taken from the file.

  python tests/golden/make_kat_gaps.py PATH/TO/vendor/spoa/test/spoa_test.cpp
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = [f"{t}{g}{q}" for t in ("Local", "Global", "SemiGlobal") for g in ("", "Affine", "Convex") for q in ("", "WithQualities")]


def read_kats(src):
    out = {}
    for name in NAMES:
        m = re.search(r"TEST_F\(SpoaTest, %s\) \{(.*?)Check\(c\);" % name, src, re.S)
        body = m.group(1)
        s = re.search(r"Setup\(AlignmentType::k(\w+), (-?\d+), (-?\d+), (-?\d+), (-?\d+), (-?\d+), (-?\d+), (\w+)\)", body)
        out[name] = dict(type=s.group(1), m=int(s.group(2)), n=int(s.group(3)), g=int(s.group(4)), e=int(s.group(5)),
                         q=int(s.group(6)), c=int(s.group(7)), quality=s.group(8) == "true",
                         consensus="".join(re.findall(r'"([ACGT]+)"', body)))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    kats = read_kats(open(sys.argv[1]).read())
    with open(os.path.join(HERE, "spoa_kat_gaps.json"), "w") as f:
        json.dump(kats, f, indent=1)
        f.write("\n")
    print(f"{len(kats)} known answers -> spoa_kat_gaps.json")


if __name__ == "__main__":
    main()
