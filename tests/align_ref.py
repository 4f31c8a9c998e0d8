"""TEST INFRASTRUCTURE: a CPU restatement of the overlap aligner (vechat_amd/csrc/vc_align.hip, entry point vc_align): the global
unit-cost alignment of a query piece against a target piece WITH the path the device code promises -- from the end cell, diagonal
first, then insertion (query base only), then deletion (target base only).  With that rule the path is unique, so the bar for
tests/test_align.py is the CIGAR string itself, byte for byte, and the distance beside it.

Plain numpy, nothing of the device code's layout: the whole (n+1) x (m+1) distance matrix in int32, filled row by row (the horizontal
pass is a prefix minimum of `new - idx`), then walked back cell by cell.  Bytes compare as bytes: case matters, 'N' equals only 'N'.
two_row_distance and cigar_cost are the independent checks tests/test_align_ref.py holds the restatement itself against.
"""
import re

import numpy as np


def matrix(q, t):
    """D[i][j] = edit distance of q[:i] and t[:j], int32, all of it"""
    qa, ta = np.frombuffer(bytes(q), np.uint8), np.frombuffer(bytes(t), np.uint8)
    n, m = len(qa), len(ta)
    idx = np.arange(m + 1, dtype=np.int32)
    D = np.empty((n + 1, m + 1), np.int32)
    D[0] = idx
    new = np.empty(m + 1, np.int32)
    for i in range(1, n + 1):
        row = D[i - 1]
        new[0] = i
        if m:
            np.minimum(row[:-1] + (ta != qa[i - 1]), row[1:] + 1, out=new[1:])
        D[i] = np.minimum.accumulate(new - idx) + idx
    return D


def traceback(D, q, t):
    """the ops from (n, m) back to (0, 0), end first: M if the diagonal explains the cell, else I if the cell above does, else D"""
    q, t = bytes(q), bytes(t)
    i, j = len(q), len(t)
    ops = []
    while i or j:
        d = int(D[i, j])
        if i and j and d == int(D[i - 1, j - 1]) + (q[i - 1] != t[j - 1]):
            ops.append("M"); i -= 1; j -= 1
        elif i and d == int(D[i - 1, j]) + 1:
            ops.append("I"); i -= 1
        else:
            assert j and d == int(D[i, j - 1]) + 1, (i, j)
            ops.append("D"); j -= 1
    return ops


def encode(ops_end_first):
    """run-length encoding, start first: <count><op>...; no ops, empty string"""
    out, run, prev = [], 0, None
    for op in reversed(ops_end_first):
        if op != prev and run:
            out.append(f"{run}{prev}"); run = 0
        prev = op; run += 1
    if run:
        out.append(f"{run}{prev}")
    return "".join(out)


def align(q, t):
    """-> (cigar, distance)"""
    D = matrix(q, t)
    return encode(traceback(D, q, t)), int(D[len(q), len(t)])


def two_row_distance(q, t):
    """the distance alone by the textbook recurrence, cell by cell in plain Python: shares nothing with matrix()"""
    q, t = bytes(q), bytes(t)
    prev = list(range(len(t) + 1))
    for qc in q:
        left = prev[0] + 1
        cur = [left]
        for tc, diag, up in zip(t, prev, prev[1:]):
            v = diag + (qc != tc)
            if up < v:
                v = up + 1
            if left < v:
                v = left + 1
            cur.append(v)
            left = v
        prev = cur
    return prev[-1]


def cigar_cost(cigar, q, t):
    """walks the CIGAR over both sequences; returns its cost, or None if it does not consume them exactly"""
    if not re.fullmatch(r"(\d+[MID])*", cigar):
        return None
    qa, ta = np.frombuffer(bytes(q), np.uint8), np.frombuffer(bytes(t), np.uint8)
    i = j = cost = 0
    for num, op in re.findall(r"(\d+)([MID])", cigar):
        n = int(num)
        if n == 0:
            return None
        if op == "M":
            if i + n > len(qa) or j + n > len(ta):
                return None
            cost += int(np.count_nonzero(qa[i:i + n] != ta[j:j + n])); i += n; j += n
        elif op == "I":
            cost += n; i += n
        else:
            cost += n; j += n
    return cost if (i, j) == (len(qa), len(ta)) else None
