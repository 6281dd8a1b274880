"""The integer schedule of the GEMM kernels, on the CPU.  gps_gemm_schedule enumerates, per
workgroup, the work items a launch would run — with the very functions the kernels call
(csrc/gemm_schedule.h: tile_of, xcd_remap, pair_of, slab_xcd_of, tile_k_range, slice_part,
small_block_of, StreamKPart) in the kernels' dispatch order — so a tile order with a hole or a
repeat, a K split that drops a remainder slice, or a stream-K run boundary that loses a slice
shows here, without a device, for every grid shape and not only the ones a GPU test runs."""
import ctypes

import numpy as np
import pytest

from gpscore import _lib

STORE, ROWSQ, COLRED = 0, 1, 2
NONE, K_LE_I, K_LE_J, K_GE_J, K_GE_I, KR_J = 0, 1, 2, 3, 4, 5
WG, TI, TJ, KB, KE, SLICE, SLOT, TICKETS = range(8)
SLOTS = 512  # 2 workgroups per CU on 256 CUs

_buf = np.zeros((1 << 16, 8), np.int32)
_plan = np.zeros(8, np.int32)


def schedule(kr=None, slots=SLOTS, **kw):
    d = dict(lay_a=0, lay_b=1, epi=STORE, M=128, N=128, K=128, alpha=1.0, beta=0.0, tri=0,
             tri_off=0, lower_out=0, mirror=0, kend=0, tile=128, ksplit=1, map_mode=0, use_ws=1,
             sk_alone=0, dep_mode=0)
    d.update(kw)
    d.update(lda=max(d["K"], d["M"]), ldb=max(d["K"], d["N"]), ldc=d["N"], ld_out=max(d["M"], d["N"]),
             c_kslice_stride=d["M"] * d["N"])
    desc = _lib.GemmDesc(**d)
    lib = _lib.load()
    krp = None if kr is None else kr.ctypes.data_as(_lib._PI)
    n = lib.gps_gemm_schedule(ctypes.byref(desc), krp, 0, slots, _plan.ctypes.data_as(_lib._PI),
                              _buf.ctypes.data_as(_lib._PI), len(_buf))
    assert 0 <= n <= len(_buf), (n, lib.gps_last_error(None), kw)
    return dict(zip(_lib.GEMM_PLAN_NAMES, (int(v) for v in _plan))), _buf[:n]


def expected_k(tri, off, ti, tj, K, tile=128):
    kb, ke = np.zeros_like(ti), np.full_like(ti, K)
    if tri == K_LE_I:
        ke = np.minimum(K, off + (ti + 1) * tile)
    elif tri == K_LE_J:
        ke = np.minimum(K, off + (tj + 1) * tile)
    elif tri == K_GE_J:
        kb = off + tj * tile
    elif tri == K_GE_I:
        kb = off + ti * tile
    return kb, np.maximum(ke, kb)


def assert_each_tile_once(items, tm, tn, lower, what):
    key = items[:, TI].astype(np.int64) * 4096 + items[:, TJ]
    ti, tj = np.meshgrid(np.arange(tm), np.arange(tn), indexing="ij")
    keep = (tj <= ti) if lower else np.ones_like(ti, bool)
    want = np.sort((ti[keep].astype(np.int64) * 4096 + tj[keep]))
    assert len(key) == len(want) and np.array_equal(np.sort(key), want), what


SIZES = list(range(1, 41)) + [63, 64, 65]
MAPS_FOR = {NONE: (0, 1, 2, 4, 5, 6), KR_J: (0, 1, 2, 4, 5, 6)}  # (5 and 6 fall back to automatic)


@pytest.mark.parametrize("tri", [NONE, K_LE_I, K_LE_J, K_GE_J, K_GE_I, KR_J])
def test_every_tile_exactly_once(tri):
    """tiles_m, tiles_n in 1..40 and {63, 64, 65}, every map launch_gemm allows for the shape,
    with and without lower_out: every tile appears exactly once (a hole of the banded maps 3 / 5
    emits nothing), in one workgroup each, with the K range its tri mode documents."""
    for tm in SIZES:
        for tn in SIZES:
            M, N = 128 * tm, 128 * tn
            off = 128 * ((tm + tn) % 3)
            K = (max(M, N) + off) if tri not in (NONE, KR_J) else 128
            kr = None
            if tri == KR_J:
                kr = np.tile(np.array([0, K], np.int32), N // 16)
                off = 0
            elif tri == NONE:
                off = 0
            for lower in ((0, 1) if tm == tn else (0,)):
                maps = MAPS_FOR.get(tri, (0, 1, 2, 3, 4, 5, 6))
                for mm in maps:
                    if mm == 3 and lower:
                        continue  # refused by launch_gemm
                    plan, it = schedule(kr, M=M, N=N, K=K, tri=tri, tri_off=off, lower_out=lower,
                                        map_mode=mm)
                    what = (tri, tm, tn, lower, mm, plan)
                    assert plan["tile"] == 128 and plan["grid_y"] == 1, what
                    assert_each_tile_once(it, tm, tn, lower, what)
                    assert len(np.unique(it[:, WG])) == len(it) and it[:, WG].max() < plan["grid_x"], what
                    kb, ke = expected_k(tri, off, it[:, TI], it[:, TJ], K)
                    assert np.array_equal(it[:, KB], kb) and np.array_equal(it[:, KE], ke), what


def test_every_tile_exactly_once_64_tiles_and_epilogues():
    """The same on 64-tiles (tile indices in units of 64) and for the reducing epilogues: the row
    norms' paired column tiles (map 6: workgroup (ri, q) runs column tile T−1−q, then q; the
    middle tile of an odd count alone) and maps 5 / 3."""
    for tm in range(1, 10):
        for tn in range(1, 10):
            for tri in (NONE, K_LE_I, K_LE_J, K_GE_J, K_GE_I):
                for mm in ((0, 1, 2, 3, 4, 5) if tri else (0, 1, 2, 4)):
                    plan, it = schedule(M=128 * tm, N=128 * tn, K=128 * max(tm, tn), tri=tri,
                                        map_mode=mm, tile=64)
                    assert plan["tile"] == 64
                    assert_each_tile_once(it, 2 * tm, 2 * tn, 0, (64, tm, tn, tri, mm))
                    kb, ke = expected_k(tri, 0, it[:, TI], it[:, TJ], 128 * max(tm, tn), 64)
                    assert np.array_equal(it[:, KB], kb) and np.array_equal(it[:, KE], ke)
    for tm in SIZES[:12] + [17, 33]:
        for tn in SIZES:
            for mm, want in ((0, 6), (6, 6), (5, 5), (1, 1)):
                off = 128 * (tn % 3)
                plan, it = schedule(M=128 * tm, N=128 * tn, K=128 * tn + off, epi=ROWSQ, tri=K_LE_J,
                                    tri_off=off, map_mode=mm)
                what = ("rowsq", tm, tn, mm, plan)
                assert plan["map_mode"] == want, what
                assert_each_tile_once(it, tm, tn, 0, what)
                kb, ke = expected_k(K_LE_J, off, it[:, TI], it[:, TJ], 128 * tn + off)
                assert np.array_equal(it[:, KB], kb) and np.array_equal(it[:, KE], ke), what
                if want == 6:
                    assert plan["grid_x"] == tm * ((tn + 1) // 2), what
                    # a workgroup's tiles: one row tile, column tiles T-1-q then q (or the middle alone)
                    order = np.argsort(it[:, WG], kind="stable")
                    s = it[order]
                    first = np.r_[True, s[1:, WG] != s[:-1, WG]]
                    second = ~first
                    prev = np.flatnonzero(second) - 1
                    assert np.array_equal(s[second, TI], s[prev, TI]), what
                    assert np.array_equal(s[second, TJ], tn - 1 - s[prev, TJ]), what
                    assert (s[second, TJ] < s[prev, TJ]).all(), what
                    assert len(np.unique(s[:, WG])) == plan["grid_x"], what
            for mm, want in ((0, 3), (5, 5), (2, 2)):
                plan, it = schedule(M=128 * tm, N=128 * tn, K=128 * tm, epi=COLRED, tri=K_LE_I,
                                    map_mode=mm)
                assert plan["map_mode"] == want
                assert_each_tile_once(it, tm, tn, 0, ("colred", tm, tn, mm))


def test_split_k_slices_partition_the_range():
    """ksplit 1..8 over 0..20 slices of 16: the slices partition [kb, ke) in order, sizes differ by
    at most one (the longer first), an empty slice is empty — through TRI_KR_J, which sets the
    tile's range freely; then the slice-major XCD deal (slab_xcd), where every (tile, slice)
    pair must appear exactly once."""
    for nk in range(0, 21):
        for ks in range(1, 9):
            for tile in (128, 64):
                kb0 = 32
                kr = np.tile(np.array([kb0, kb0 + 16 * nk], np.int32), 128 // 16)
                plan, it = schedule(kr, M=128, N=128, K=kb0 + 16 * 20 + 16, tri=KR_J, tile=tile, ksplit=ks)
                ntile = (128 // tile) ** 2
                assert (plan["ksplit"], plan["grid_y"], len(it)) == (ks, ks, ks * ntile), (nk, ks, plan)
                for t in range(ntile):
                    s = it[(it[:, TI] * 2 + it[:, TJ]) == (t // (128 // tile)) * 2 + t % (128 // tile)]
                    s = s[np.argsort(s[:, SLICE])]
                    assert np.array_equal(s[:, SLICE], np.arange(ks))
                    assert s[0, KB] == kb0 and s[-1, KE] == kb0 + 16 * nk, (nk, ks, s)
                    assert np.array_equal(s[1:, KB], s[:-1, KE]), (nk, ks, s)
                    n = (s[:, KE] - s[:, KB]) // 16
                    assert (np.diff(n) <= 0).all() and n.max() - n.min() <= 1, (nk, ks, n)
    for (tm, tn, lower) in ((2, 3, 0), (5, 5, 1), (7, 9, 0), (13, 13, 1)):
        for ks in range(2, 9):
            for nk in (1, 3, ks, 2 * ks + 1):
                plan, it = schedule(M=128 * tm, N=128 * tn, K=16 * nk, ksplit=ks, lower_out=lower)
                assert plan["slab_xcd"] == 1 and plan["grid_y"] == ks, plan
                ntile = tm * (tm + 1) // 2 if lower else tm * tn
                key = (it[:, TI].astype(np.int64) * 4096 + it[:, TJ]) * 16 + it[:, SLICE]
                assert len(it) == ntile * ks and len(np.unique(key)) == len(it), (tm, tn, ks, nk)
                assert len(np.unique(it[:, WG])) == len(it)
                assert (it[:, KE] - it[:, KB]).sum() == ntile * 16 * nk
                for sl in range(ks):
                    assert_each_tile_once(it[it[:, SLICE] == sl], tm, tn, lower, (tm, tn, ks, sl))


def check_stream_k(tiles, nk, lower_tm=0):
    if lower_tm:
        kw = dict(M=128 * lower_tm, N=128 * lower_tm, lower_out=1)
        tm, tn = lower_tm, lower_tm
    else:
        kw = dict(M=128, N=128 * tiles)
        tm, tn = 1, tiles
    K = 16 * nk
    plan, it = schedule(K=K, sk_alone=1, **kw)
    rem = tiles % SLOTS
    what = (tiles, nk, plan)
    if rem == 0 or 4 * rem > 3 * SLOTS:  # launch_gemm: a last round more than 3/4 full runs as it is
        assert plan["sk_wgs"] == 0 and plan["grid_x"] == tiles, what
        assert_each_tile_once(it, tm, tn, bool(lower_tm), what)
        return
    assert plan["sk_dp"] == tiles - rem and plan["sk_wgs"] == min(SLOTS, rem * nk), what
    assert plan["grid_x"] == plan["sk_dp"] + plan["sk_wgs"], what
    whole = it[it[:, SLOT] < 0]
    part = it[it[:, SLOT] >= 0]
    assert (whole[:, KB] == 0).all() and (whole[:, KE] == K).all() and (whole[:, TICKETS] == 0).all(), what
    key = lambda a: a[:, TI].astype(np.int64) * 4096 + a[:, TJ]
    # whole tiles and partial tiles are disjoint, together every tile once
    pk, inv, cnt = np.unique(key(part), return_inverse=True, return_counts=True)
    assert not np.intersect1d(pk, key(whole)).size, what
    ti, tj = np.meshgrid(np.arange(tm), np.arange(tn), indexing="ij")
    keep = (tj <= ti) if lower_tm else np.ones_like(ti, bool)
    want = np.sort(ti[keep].astype(np.int64) * 4096 + tj[keep])
    assert np.array_equal(np.sort(np.r_[key(whole), pk]), want), what
    assert len(pk) + np.count_nonzero(whole[:, WG] >= plan["sk_dp"]) == rem, what
    # the runs of a partial tile partition [0, K)
    order = np.lexsort((part[:, KB], inv))
    s, g = part[order], inv[order]
    start = np.r_[True, g[1:] != g[:-1]]
    end = np.r_[start[1:], True]
    assert (s[start, KB] == 0).all() and (s[end, KE] == K).all(), what
    assert np.array_equal(s[1:, KB][~start[1:]], s[:-1, KE][~end[:-1]]), what
    assert (s[:, KE] > s[:, KB]).all(), what
    # workspace slots: pairwise distinct, within the (remainder + slots) tiles launch_gemm checks
    assert len(np.unique(part[:, SLOT])) == len(part) and part[:, SLOT].max(initial=0) < rem + SLOTS, what
    # the ticket count the last arriver waits for is the number of contributors (first ticket is 0)
    assert np.array_equal(part[:, TICKETS], cnt[inv] - 1), what
    # contributors are consecutive workgroups (the combine reads slots u + s0 .. u + s1)
    assert np.array_equal(s[1:, WG][~start[1:]], s[:-1, WG][~end[:-1]] + 1), what


@pytest.mark.parametrize("lo,hi", [(513, 660), (660, 807), (807, 954), (954, 1101)])
def test_stream_k_partition(lo, hi):
    """Tiles 513..1100 (in four parts) with 2..40 slices of K on 512 slots: the runs partition every (tile,
    slice) of the tail, workspace slots are distinct and within capacity, and every combined
    tile's ticket count equals its number of partial contributors.  (Tails with fewer slices than
    slots — small K — were cut into runs that were mostly empty before this test existed, which
    broke the last two properties: launch_gemm now starts at most one workgroup per slice.)"""
    for tiles in range(lo, hi):
        for nk in range(2, 41):
            check_stream_k(tiles, nk)
    for tm in (32, 33, 36, 40, 45):  # lower_out: tm(tm+1)/2 tiles in tile_of's triangular order
        for nk in (2, 3, 7, 32, 40):
            check_stream_k(tm * (tm + 1) // 2, nk, lower_tm=tm)


@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("waves", [1, 2, 4])
def test_small_kernel_blocks(tile, waves):
    """The small kernel's enumeration: every block once per wave part, with lower_out exactly the
    blocks of the lower 64-tiles (its prefix search); the waves' shares partition the K range."""
    u = 64 // tile
    for M in range(128, 1281, 128):
        for (N, lower) in ((M, 1), (M, 0), (384, 0)):
            for (tri, K) in ((NONE, 80), (K_LE_I, M), (K_GE_J, max(M, N))):
                plan, it = schedule(M=M, N=N, K=K, tile=tile, ksplit=waves, lower_out=lower, tri=tri)
                assert (plan["tile"], plan["ksplit"]) == (tile, waves)
                ti, tj = np.meshgrid(np.arange(M // tile), np.arange(N // tile), indexing="ij")
                keep = (tj // u <= ti // u) if lower else np.ones_like(ti, bool)
                nblk = int(keep.sum())
                assert plan["grid_x"] == (nblk * waves + 3) // 4
                for part in range(waves):
                    s = it[it[:, SLICE] == part]
                    k = np.sort(s[:, TI].astype(np.int64) * 4096 + s[:, TJ])
                    assert np.array_equal(k, np.sort(ti[keep].astype(np.int64) * 4096 + tj[keep])), \
                        (tile, waves, M, N, lower, part)
                order = np.lexsort((it[:, SLICE], it[:, TJ], it[:, TI]))
                s = it[order].reshape(nblk, waves, 8)
                kb, ke = expected_k(tri, 0, s[:, 0, TI], s[:, 0, TJ], K, tile)
                assert np.array_equal(s[:, 0, KB], kb) and np.array_equal(s[:, -1, KE], ke)
                assert np.array_equal(s[:, 1:, KB], s[:, :-1, KE])
                assert (s[:, :, WG] == s[:, :1, WG]).all()  # a block's parts share a workgroup
