#!/usr/bin/env python3
"""Exhaustive LDS bank check of the F(4,3) x F(4,3) tile's maps (csrc/conv3d_wino44.hip), per
MI355X_MICROARCH.md's LDS table, for both tile geometries (w44::Geo<8>: 32 x 2, and w44::Geo<4>:
16 x 4): the V-pass's halo reads in both forms the compiler gives them -- a0 / a1 paired into a
ds_read2_b64 (two accesses, 16-lane groups, 32 banks), a2 a ds_read_b64 (two 32-lane groups, 64
banks); each of the three reads is checked in both forms, so the result does not hang on which
loads get paired -- its ds_write_b128 of V (groups of 8 lanes, 32 banks) and the steps'
ds_read_b128 of V (the four 16-lane groups, 64 banks), every kh, x-half, read offset and plane.
For the wide geometry also, for the record, forms the code no longer has: the reads as the
ds_read2_b32 they compiled to while loaded through HIP's float2 struct (32-lane groups, 32 banks:
the round-6 PMC's 30 M conflict cycles per launch), and the b64 tail accesses.  Prints the extra
cycles per instruction (0 = conflict-free); exits 1 if a map of the current code has any."""
import sys

CB = [1, 1027, 2081, 3107]
B128_GROUPS = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS]


class Geo:
    """w44::Geo<Q>: Q W groups x 16 / Q rows per tile plane"""

    def __init__(self, q):
        self.Q, self.TW, self.TH = q, 4 * q, 16 // q
        self.RH, self.RWA = self.TH + 2, self.TW + 8
        self.RSLOTS = self.RH if q == 8 else self.RH + 1
        self.PLANEA = self.RSLOTS * self.RWA
        self.GS, self.XHS, self.TRS = 40, 20, 40 * q
        self.TCS = 1284 if q == 8 else 964

    def row_slot(self, r):
        """staged slot of halo row r: the narrow tile leaves the slot before its last row empty"""
        return r if self.Q == 8 or r < self.RH - 1 else r + 1

    def vpass_unit(self, t):
        """thread -> (W group, channel, halo row, x-half)"""
        if self.Q == 8:
            g = (t & 3) | (((t >> 3) & 1) << 2)
            c = ((t >> 2) & 1) | (((t >> 4) & 1) << 1)
            return g, c, (t >> 5) & 3, t >> 7
        hw = (t >> 5) & 3
        ub = 0 if hw == 3 else hw  # the fourth half-wave of an x-half repeats the first one's units
        rb = (t >> 3) & 1
        c = ((t >> 2) & 1) | (((t >> 4) & 1) << 1)
        return t & 3, c, (ub + 2 * rb) if ub < 2 else 4 + rb, t >> 7

    def halo(self, t, pl, j):
        g, c, r, _ = self.vpass_unit(t)
        return CB[c] + pl * self.PLANEA + self.row_slot(r) * self.RWA + 3 + 4 * g + 2 * j

    def v_write(self, t, m):
        g, c, r, xh = self.vpass_unit(t)
        return c * self.TCS + r * self.TRS + g * self.GS + xh * self.XHS + 4 * m

    def v_read(self, l, xh, kh, off):
        ci, p = l >> 4, l & 15
        return ci * self.TCS + (p // self.Q + kh) * self.TRS + self.GS * (p % self.Q) + self.XHS * xh + off


def conflicts(addrs_by_group, width, banks):
    """extra LDS cycles: per group, the max number of distinct dword addresses on one bank - 1"""
    extra = 0
    for addrs in addrs_by_group:
        per_bank = {}
        for a in set(addrs):
            for k in range(width):
                per_bank.setdefault((a + k) % banks, set()).add(a + k)
        extra += max(len(v) for v in per_bank.values()) - 1
    return extra


def check(geo):
    """the current code's maps: extra cycles of (V-pass reads as ds_read_b64 + V writes, V-pass
    reads as ds_read2_b64, step reads)"""
    units = {geo.vpass_unit(t) for t in range(256)}
    assert units == {(g, c, r, xh) for g in range(geo.Q) for c in range(4) for r in range(geo.RH) for xh in range(2)}, \
        "the V-pass covers every (group, channel, row, x-half)"
    assert geo.PLANEA * 6 // 4 <= 4 * 64 and geo.PLANEA * 6 <= CB[1] - CB[0], "whole pieces per channel region"
    assert geo.TRS >= geo.Q * geo.GS and geo.TCS >= geo.RH * geo.TRS, "V rows and channels do not overlap"
    worst, pair = 0, 0
    for wave in range(4):
        lanes = range(64 * wave, 64 * wave + 64)
        assert len({geo.vpass_unit(t)[3] for t in lanes}) == 1, "the x-half is wave-uniform"
        for pl in range(6):
            for j in range(3):  # the three b64 reads per plane
                addr = {t % 64: geo.halo(t, pl, j) for t in lanes}
                assert all(a % 2 == 0 for a in addr.values()), "b64 alignment"
                e = conflicts([[addr[l] for l in range(0, 32)], [addr[l] for l in range(32, 64)]], 2, 64)
                worst = max(worst, e)
                # one access of a ds_read2_b64: the four 16-lane groups on 32 banks
                e = conflicts([[addr[l] for l in range(16 * k, 16 * k + 16)] for k in range(4)], 2, 32)
                pair = max(pair, e)
        for m in range(5):  # the V-pass's b128 writes (the fifth: floats 16, 17 + slot padding)
            addr = {t % 64: geo.v_write(t, m) for t in lanes}
            assert all(a % 4 == 0 for a in addr.values()), "b128 alignment"
            e = conflicts([[addr[l] for l in range(8 * k, 8 * k + 8)] for k in range(8)], 4, 32)
            worst = max(worst, e)
    steps = 0
    for xh in range(2):
        for kh in range(3):
            for m in range(5):
                addr = {l: geo.v_read(l, xh, kh, 4 * m) for l in range(64)}
                assert all(a % 4 == 0 for a in addr.values())
                steps = max(steps, conflicts([[addr[l] for l in g] for g in B128_GROUPS], 4, 64))
    return worst, pair, steps


def history(geo):
    """forms the wide geometry's code had before its fixes, for the record"""
    w32, wb64 = 0, 0
    for wave in range(4):
        lanes = range(64 * wave, 64 * wave + 64)
        for pl in range(6):
            for j in range(3):
                addr = {t % 64: geo.halo(t, pl, j) for t in lanes}
                for k in range(2):  # each dword alone, as ds_read_b32 / one half of ds_read2_b32
                    w32 = max(w32, conflicts([[addr[l] + k for l in range(0, 32)], [addr[l] + k for l in range(32, 64)]], 1, 32))
        addr = {t % 64: geo.v_write(t, 4) for t in lanes}
        wb64 = max(wb64, conflicts([[addr[l] for l in range(16 * k, 16 * k + 16)] for k in range(4)], 2, 32))
    print("V-pass halo reads as ds_read_b32 / ds_read2_b32 (the pre-fix code): extra cycles per access", w32)
    print("V-pass V b64 write (the pre-fix tail store): extra cycles", wb64)
    worst = 0
    for xh in range(2):
        for kh in range(3):
            addr = {l: geo.v_read(l, xh, kh, 16) for l in range(64)}
            worst = max(worst, conflicts([[addr[l] for l in range(0, 32)], [addr[l] for l in range(32, 64)]], 2, 64))
    print("step V tail read as ds_read_b64 (pre-fix): extra cycles", worst)
    worst = 0
    for xh in range(2):
        for kh in range(2):  # two kh rows paired into one ds_read2_b64 (16-lane groups, 32 banks)
            addr = {l: geo.v_read(l, xh, kh, 16) for l in range(64)}
            worst = max(worst, 2 * conflicts([[addr[l] for l in range(16 * k, 16 * k + 16)] for k in range(4)], 2, 32))
    print("step V tail reads as ds_read2_b64 (pre-fix, both accesses): extra cycles", worst)


def main():
    bad = 0
    for q in (8, 4):
        geo = Geo(q)
        print(f"-- {geo.TW} x {geo.TH} tile (Q = {q}): rows of {geo.RWA} floats, planes {geo.PLANEA} apart, "
              f"V [ci: {geo.TCS}][row: {geo.TRS}][group: {geo.GS}][x-half: {geo.XHS}]")
        vp, pair, steps = check(geo)
        print("V-pass halo reads (ds_read_b64) + V b128 writes: extra cycles", vp)
        print("V-pass halo reads as ds_read2_b64 (a0 / a1 in the assembly): extra cycles per access", pair)
        print("step V reads (ds_read_b128): extra cycles", steps)
        bad += vp + pair + steps
        if q == 8:
            history(geo)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
