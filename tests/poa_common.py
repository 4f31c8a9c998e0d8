"""What the tests/test_poa*.py files share: the alignment types and gap models by name, gap parameters, the size of a process
pool, poa_*'s keywords for a tuple of scores, and the `done` lines of a VC_LARGE_LOG capture."""
import os
import re

from vechat_amd import capi

TYPES = {"SW": 0, "NW": 1, "OV": 2}
MODELS = {"linear": (5, -4, -8, -8, -8, -8), "affine": (5, -4, -8, -6, -8, -6), "convex": (5, -4, -8, -6, -10, -4)}


def _gp(**kw):
    p = capi.VcPoaGapParams(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-6, gap_open2=-10, gap_extend2=-4)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _workers():
    return max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))


def _kw(scores):
    m, n, g, e, q, c = scores
    return dict(match=m, mismatch=n, gap=g, gap_extend=e, gap_open2=q, gap_extend2=c)


def _done(err):
    """-> [(alignments, cells)] of the "vc_large: done" lines of a stderr capture"""
    return [tuple(map(int, re.match(r"vc_large: done alignments=(\d+) cells=(\d+)", l).groups()))
            for l in err.splitlines() if l.startswith("vc_large: done")]
