"""A numpy model of the batch with an automatic center per capture (urh_amd/csrc/batch_center.hip), capture by capture: the oracle's
demodulation (gated with the capture's own threshold), detect_center's histogram (center_cases.histogram), the flag rules of
include/urhgpu.h (0 none, 1 decided, 2 more bins than the pool holds, 3 the second and third peak tie), the peak picking
(numpy_estimators.center_from_histogram, which walks np.argsort's order as the reference does), the slicing thresholds
(urh_amd.batch.center_thresholds: k_batch_center_publish's arithmetic) and the slicing.  No GPU."""
from dataclasses import replace

import numpy as np

import center_cases as cc
import noise_cases as nc
import numpy_estimators as ne


def center_of(qad, max_size, pool_bins=cc.POOL_BINS):
    """(flag the device reports, center the method hands out: a float or None)"""
    h = cc.histogram(qad, max_size)
    if h is None:
        return 0, None
    y, edges = h
    c = ne.center_from_histogram(y, edges)
    if len(y) > pool_bins:
        return 2, None if c is None else float(c)
    peaks = cc.strict_peaks(y)
    if not peaks:
        assert c is None
        return 0, None
    counts = sorted((int(y[i]) for i in peaks), reverse=True)
    return (3 if len(counts) >= 3 and counts[1] == counts[2] else 1), float(c)


def capture(oracle, iq, p, max_size, auto_noise=True, pool_bins=cc.POOL_BINS):
    """{noise, noise_flag, flag, center, thresholds, qad, pp, flat} of one capture of the batch"""
    thr, nflag = (p.noise_threshold, 1)
    if auto_noise:
        thr, nflag = nc.oracle_threshold(oracle, iq)
    if nflag == 0:
        return dict(noise=thr, noise_flag=0)
    if nflag == 2:
        qad = np.zeros(2, np.float32)                       # Signal.py:474-484
    else:
        qad = cc.demodulated(oracle, iq, replace(p, noise_threshold=thr))
    flag, center = center_of(qad, max_size, pool_bins)
    from urh_amd.batch import center_thresholds
    thresholds = center_thresholds(p, [center])[0]
    pp, flat = nc.slice_qad(oracle, qad, replace(p, write_bit_sample_pos=True), center)
    return dict(noise=thr, noise_flag=nflag, flag=flag, center=center, thresholds=thresholds, qad=qad, pp=pp, flat=flat)


def plan(k, total, max_bins):
    """urhgpu_batch_center_plan restated: (scratch bytes, groups, captures per group)"""
    up = lambda x: (x + 255) & ~255                         # noqa: E731
    group = max(1, (64 << 20) // (4 * max_bins))
    kg = min(k, group)
    nt = max(total, 0) // 4096 + kg + 1
    nm = kg + 1
    state_bytes = 168                                       # sizeof(MsgState): 21 eight-byte fields
    o = 0
    for part in (nm * state_bytes, nt * 8, (nt + 1) * 8, nt * 8, (nt + 1) * 4, nt * 32 * 4, max(total, 1) * 4, nm * 4):
        o = up(o + part)
    o = up(o + up(nm * max_bins * 4 + 256) + nt * 4)
    return o, -(-k // group), group
