"""Helpers shared by the parity tests and the host-side tests."""
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'transcar_hip.h')


def header_text(comments=True):
    """include/transcar_hip.h; comments=False: without its /* ... */ comments"""
    text = open(HEADER).read()
    return text if comments else re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def header_define(name):
    """the value of `#define name <integer expression>`: 12288, (1 << 20)"""
    m = re.search(r'^#define %s\s+(.+?)\s*$' % name, header_text(), flags=re.M)
    assert m, name
    return int(eval(m.group(1), {'__builtins__': {}}))


def header_functions():
    """the sorted names of the tc_* functions the header declares"""
    return sorted(set(re.findall(r'\b(tc_[a-z0-9_]+)\s*\(', header_text(comments=False))))


def assert_rows_match(a, b, atol, what='rows'):
    """a, b: [n, d].  Every row of ``b`` must have a distinct partner row in
    ``a`` within ``atol`` (max-abs): equal up to a permutation.  Used for
    top-k outputs, where near-tied scores may swap neighbours."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    used = np.zeros(len(a), dtype=bool)
    for i in range(len(b)):
        d = np.abs(a - b[i]).max(axis=1)
        d[used] = np.inf
        j = int(np.argmin(d))
        assert d[j] <= atol, '%s: row %d has no partner (best %.3g)' % (
            what, i, d[j])
        used[j] = True


def frac_within(a, b, atol):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) <= atol).mean())
