"""The pose estimators' workspace row (csrc/pose_device.hpp) as the oracles pose_detector_ref.py / pose_icp_ref.py and the sweeps
under tests/randomised see it: the in-order fp32 sum, the triangle's unpacking, the order-free bound (docs/ORACLE_PINS.md)."""

import numpy as np

EPS = 2.0 ** -24


def reduce_rows(rows):
    """([28] fp32 sums, count) of workspace rows [n, 32], added in fp32 in workgroup order as the step kernels add them"""
    acc = np.zeros(28, np.float32)
    for r in rows:
        acc = (acc + r[:28]).astype(np.float32)
    return acc, int(rows[:, 28].view(np.int32).sum())


def unpack_row(row):
    """[>= 27] -> (the symmetric [6, 6] of words 0..20, words 21..26) in float64"""
    row = np.asarray(row, np.float64)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = row[:21]
    return A + np.triu(A, 1).T, row[21:27]


def row_bound(n_terms, row_abs, roundings):
    """a sum of n_terms fp32 terms, in any order, each term ``roundings`` roundings from exact: (N + roundings) 2^-24 sum |term|"""
    return (n_terms + roundings) * EPS * np.asarray(row_abs)
