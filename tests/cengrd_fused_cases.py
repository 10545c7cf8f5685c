"""Inputs shared by tests/test_gpu_cengrd_fused.py (GPU) and tests/test_cengrd_fused_inputs.py (CPU): the wide pair that drives the row
engine past its strip capacity, and hand-made planes for cspm_plane_cost_batch whose taps reach the pad columns and leave the
disparity range.  Nothing here imports the GPU library."""
import functools

import numpy as np

from crossscalepatchmatch_amd import synth
from oracle import pyoracle as po

# ---- the wide pair ------------------------------------------------------------------------------------------------------------
# cspm_rows.h: a wave's other-view strip holds strip_capacity(max_dis, half) = min(64 + 2 * half + max_dis + 2, 384) slots, and a level
# pass is staged through LDS when the strip it needs -- (cmax - cmin) + 2 * half + D + 1 slots for the left view, one more for the
# right view -- fits.  A full wave has cmax - cmin = 63; with the 35-wide window (half = 17):
#   max_dis = 250: capacity 350, a full wave needs 348 / 349 slots          -> STAGED (all six staging registers per lane in use)
#   max_dis = 300: capacity 384 (saturated), a full wave needs 398 / 399    -> both views read from global memory; the last wave of a
#                  352-pixel row owns 32 pixels (needs 366 / 367) and stays staged: both paths run in one launch
# The switch is at max_dis = 284 (capacity 384, needs 382 / 383).
WIDE_W, WIDE_H, WIDE_WND = 352, 40, 35
WIDE_STAGED_D, WIDE_GLOBAL_D = 250, 300
K_STRIP_SLOTS = 384  # kStripRegs * kWave


def strip_capacity(max_dis, half):
    return min(64 + 2 * half + max_dis + 2, K_STRIP_SLOTS)


def full_wave_strip(max_dis, half, view):
    """slots a wave of 64 adjacent centres needs of the other view (level_rows: s_len)"""
    return 63 + 2 * half + max_dis + 1 + (1 if view == 1 else 0)


@functools.lru_cache(maxsize=None)
def wide_images():
    """352x40 noise texture with true disparities below 60: matching cells exist at either max_dis"""
    l, r, _, _ = synth.make_pair(WIDE_W, WIDE_H, 60, regions=3, seed=41)
    return l, r


# ---- hand-made planes for cspm_plane_cost_batch ----------------------------------------------------------------------------------
def hand_planes(w, h, D):
    """(xy, norm, param): fronto-parallel and slanted planes at the left and right image border and in the middle, with disparities
    inside the range (their other-view columns x - d / x + d leave the image near the border: pad cells, H = 80 and the border
    branch of G), and below 1 / at and above D (the max_cost branch)"""
    ys = [0, h // 2, h - 1]
    xs = [0, 1, 8, w // 2, w - 9, w - 2, w - 1]
    zs = [1.0, 2.5, D / 2 + 0.25, D - 1.0, D - 0.5, 0.5, -3.0, float(D), D + 6.75]
    norms = [(0.0, 0.0, 1.0), (0.05, 0.0, 1.0), (-0.05, 0.02, 1.0)]
    xy, norm, point = [], [], []
    for y in ys:
        for x in xs:
            for z in zs:
                for n in norms:
                    xy.append((x, y))
                    norm.append(np.array(n) / np.linalg.norm(n))
                    point.append((float(x), float(y), z))
    xy = np.array(xy, np.int32)
    norm = np.array(norm)
    param = np.stack([po.plane_param(norm[i], np.array(point[i])) for i in range(len(xy))])
    return xy, norm, param


def tap_counts(xy, param, w, h, D, view, wnd=35):
    """level-0 taps of the planes' windows, counted with the reference's tap rule (pre_cs_pc.cc:155-175): taps inside the image whose
    disparity static_cast<int>(a * x + b * y + c) lies outside [1, D - 1] (the max_cost branch), and valid taps whose other-view
    column x -+ f or x -+ (f + 1) is a pad column on the left / on the right of the other image (the left view only ever reaches the
    left pad, the right view the right pad; the other border is reached by the window itself: own_left / own_right)"""
    half = wnd // 2
    out_of_range = pad_left = pad_right = own_left = own_right = 0
    for (cx, cy), (a, b, c) in zip(xy, param):
        x = np.arange(cx - half, cx + half + 1)
        own_left += int(np.sum(x < 0))  # window columns beyond the own image: masked taps, the own element is a pad cell
        own_right += int(np.sum(x >= w))
        y = np.arange(cy - half, cy + half + 1)
        x = x[(x >= 0) & (x < w)]
        y = y[(y >= 0) & (y < h)]
        q = a * x[None, :] + (b * y[:, None] + c)
        with np.errstate(invalid="ignore"):
            f = np.trunc(np.clip(q, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
        valid = (f >= 1) & (f <= D - 1)
        out_of_range += int(np.sum(~valid))
        sign = -1 if view == 0 else 1
        for step in (0, 1):
            xo = x[None, :] + sign * (f + step)
            pad_left += int(np.sum(valid & (xo < 0)))
            pad_right += int(np.sum(valid & (xo >= w)))
    return dict(out_of_range=out_of_range, pad_left=pad_left, pad_right=pad_right, own_left=own_left, own_right=own_right)
