#!/usr/bin/env python3
"""Exhaustive LDS bank check of the right head's staged kernel (csrc/disparity_right.hip), per
MI355X_MICROARCH.md's LDS table: per wave, tile phase (xr0 mod 3) and candidate od, the four
taps as the two ds_read2_b32 the compiler emits (each dword a ds_read_b32: 32-lane groups,
32 banks), the per-column table entry as ds_read_b64 (32-lane groups, 64 banks) and the
per-od table entry (one address per wave: a broadcast).  The axes are the ideal x3 ones
(i0 = (x - 1) // 3, k0 = (od - 1) // 3).  Prints the extra cycles (0 = conflict-free)."""
K_R_COLS = 92
THREADS = 256


def extra(addrs, banks):
    per_bank = {}
    for a in set(addrs):
        per_bank.setdefault(a % banks, set()).add(a)
    return max(len(v) for v in per_bank.values()) - 1


def main():
    worst_tap = worst_col = 0
    for d3 in (4, 8, 16, 32, 64, 88):
        for phase in range(3):            # xr0 = 256 * blockIdx.x: every residue mod 3 occurs
            xr0 = 256 * phase
            c0 = xr0 // 3
            for od in range(3 * d3):
                off = max(od - 1, 0) // 3 * (K_R_COLS - 1)
                for wave in range(THREADS // 64):
                    for half in range(2):
                        lanes = range(64 * wave + 32 * half, 64 * wave + 32 * half + 32)
                        base = [off + max(xr0 + t + od - 1, 0) // 3 - c0 + 2 for t in lanes]
                        for tap in (0, 1, K_R_COLS - 1, K_R_COLS):
                            worst_tap = max(worst_tap, extra([b + tap for b in base], 32))
                        col = [2 * (t + od) + w for t in lanes for w in (0, 1)]  # RCol: two dwords
                        worst_col = max(worst_col, extra(col, 64))
    print("taps (ds_read2_b32): extra cycles", worst_tap)
    print("column table (ds_read_b64): extra cycles", worst_col)
    return worst_tap + worst_col


if __name__ == "__main__":
    raise SystemExit(1 if main() else 0)
