#!/usr/bin/env python
"""CPU model of the LDS bank conflicts of the radius-4 window lookup (mac-vo_amd/csrc/corr_lookup.hip): the tap phase's four cell reads and
two axis-entry reads, the staging stores, the result stores and the reads of the transposed global store — for the layout up to this
change ("old": 64 consecutive (tap, query) pairs per round, tj fastest; block row stride 12 / 18; results in one outs[81][QPB + 1]) and the
present one ("new": round r = query r with lane = 8 ti + tj, leftover column / row of two queries per extra round; row stride 12 / 20, blocks
18 banks apart; results in per-wave strips of 82 / 83 floats per query).

Bank rules (MI355X): a 4-byte LDS access is served in two groups of 32 lanes, bank = dword address mod 32; an 8-byte read in two groups of 32 lanes,
bank = dword address mod 64 (each lane takes two neighbouring banks); 8-byte stores go in four groups of 16 lanes, bank = dword address mod 32.  Lanes of a
group that read the same address are one access (broadcast); every further distinct address on a busy bank costs the group one more
cycle.  Reported per instruction stream: LDS-array cycles without conflicts, extra cycles from conflicts, and their ratio
extra / (base + extra) — the quantity SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE measures.

    python profiles/probes/lookup_lds_bank_model.py            # table for both kernels, QPW = 2 and 4
The block offsets (cx, cy) of a query's window in its staged block are 1, 1 in the row-major kernel (always, up to the rare rounding case) and
1 + (x mod 4), 1 + (y mod 4) in the tiled one: the tiled figures are averaged over all offsets of the two queries that share a leftover round."""
import itertools
import sys

K, KK = 9, 81


def pitch(qpw):          # strip_pitch<9, QPW>() and the padding of wave_floats<9, QPW, CELLS>() in the source
    return 83 if qpw == 4 else 82


def wave_pad(qpw):
    return 12 if qpw == 4 else 0


def group_cycles(accesses, nbanks, width=1):
    """accesses: (dword address) per live lane of ONE lane group -> (1, extra cycles).  width = dwords per lane."""
    per_bank = {}
    for a in set(accesses):
        for d in range(width):
            per_bank.setdefault((a + d) % nbanks, set()).add(a + d)
    worst = max((len(v) for v in per_bank.values()), default=1)
    return 1, worst - 1


def stream(lanes_addr, nbanks=32, width=1, group=32):
    """lanes_addr: list of 64 entries (dword address or None for an idle lane) -> (base, extra) LDS-array cycles of one wave instruction."""
    base = extra = 0
    for g0 in range(0, 64, group):
        acc = [a for a in lanes_addr[g0:g0 + group] if a is not None]
        if not acc:
            continue
        b, e = group_cycles(acc, nbanks, width)
        base, extra = base + b, extra + e
    return base, extra


def deal_old(qpw):
    """rounds of 64 lanes -> (s, ti, tj, live) per lane"""
    npair = qpw * KK
    rounds = []
    for r in range((npair + 63) // 64):
        row = []
        for lane in range(64):
            pair = min(r * 64 + lane, npair - 1)
            s, tap = divmod(pair, KK)
            ti, tj = divmod(tap, K)
            row.append((s, ti, tj, r * 64 + lane < npair))
        rounds.append(row)
    return rounds


def deal_new(qpw):
    rounds = [[(r, lane >> 3, lane & 7, True) for lane in range(64)] for r in range(qpw)]
    for m in range(qpw // 2):
        row = []
        for lane in range(64):
            l, rowh = lane & 31, lane >= 32
            sl = (1 if l >= 9 else 0) if rowh else (l >> 3) & 1
            ti = min(l - 9 * sl, 8) if rowh else 8
            tj = 8 if rowh else l & 7
            row.append((2 * m + sl, ti, tj, l < 18 if rowh else l < 16))
        rounds.append(row)
    return rounds


def tap_reads(rounds, stride, cells, offs, ax_base=0):
    """offs[s] = (cx, cy) of query s -> summed (base, extra) of the 4 cell reads and of the 2 axis reads of a wave's tap phase"""
    cb = ce = ab = ae = 0
    for row in rounds:
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            b, e = stream([s * cells + (tj + offs[s][1] + dy) * stride + ti + offs[s][0] + dx for s, ti, tj, _ in row])
            cb, ce = cb + b, ce + e
        for sel in (0, 1):   # AxisEntry = 2 dwords, entry index s * 18 + (ti | 9 + tj)
            b, e = stream([ax_base + 2 * (s * 2 * K + (ti if sel == 0 else K + tj)) for s, ti, tj, _ in row], nbanks=64, width=2)
            ab, ae = ab + b, ae + e
    return cb, ce, ab, ae


def staging_stores(kind, new, qpw):
    """(base, extra) of the stores that put one wave's cell blocks into LDS"""
    b = e = 0
    if kind == "row":
        cells = 146 if new else 144
        for s in range(qpw):
            for k in range(2):      # the two inner-row loads of 60 lanes; (the margin store of 24 lanes is contiguous as well)
                bb, ee = stream([s * cells + 12 + k * 60 + lane if lane < 60 else None for lane in range(64)])
                b, e = b + bb, e + ee
    else:
        bsp, cells = (20, 338) if new else (18, 288)
        for s in range(qpw):
            for k in range(4):      # fp32 cells: lane = (tile column, cell of the tile), one tile row per store
                bb, ee = stream([s * cells + (4 * k + ((lane & 15) >> 2)) * bsp + 4 * (lane >> 4) + (lane & 3) for lane in range(64)])
                b, e = b + bb, e + ee
    return b, e


def result_stores(rounds, new, qpw, qpb, wave=0):
    b = e = 0
    for row in rounds:
        if new:
            addr = [s * pitch(qpw) + (8 * ti + tj if tj < 8 else 72 + ti) if live else None for s, ti, tj, live in row]
        else:
            addr = [(ti * K + tj) * (qpb + 1) + wave * qpw + s if live else None for s, ti, tj, live in row]
        bb, ee = stream(addr)
        b, e = b + bb, e + ee
    return b, e


def final_reads(new, qpw, qpb, blk_stride):
    """the transposed store's LDS reads: idx = t, t + NTHR, ... over 81 * QPB; (base, extra) per workgroup"""
    nthr = 64 * (qpb // qpw)
    b = e = 0
    for w0 in range(0, KK * qpb, 64):
        addr = []
        for idx in range(w0, w0 + 64):
            if idx >= KK * qpb:
                addr.append(None)
                continue
            u, c = divmod(idx, qpb)
            addr.append((c // qpw) * blk_stride + (c % qpw) * pitch(qpw) + u if new else u * (qpb + 1) + c)
        bb, ee = stream(addr)
        b, e = b + bb, e + ee
    return b, e, nthr


def report(kind, qpw, qpb):
    out = []
    for new in (False, True):
        rounds = deal_new(qpw) if new else deal_old(qpw)
        if kind == "row":
            stride, cells = 12, (146 if new else 144)
            offsets = [[(1, 1)] * qpw]
        else:
            stride, cells = (20, 338) if new else (18, 288)
            pair = list(itertools.product(range(1, 5), repeat=4))          # (cx, cy) of two neighbouring queries, every combination
            offsets = [[(p[0], p[1]), (p[2], p[3])] * (qpw // 2) for p in pair]
        acc = [0, 0, 0, 0]
        for offs in offsets:
            for i, v in enumerate(tap_reads(rounds, stride, cells, offs)):
                acc[i] += v / len(offsets)
        sb, se = staging_stores(kind, new, qpw)
        rb, re_ = result_stores(rounds, new, qpw, qpb)
        fb, fe, _ = final_reads(new, qpw, qpb, qpw * cells + (wave_pad(qpw) if new else 0))
        nwave = qpb // qpw
        fb, fe = fb / nwave, fe / nwave                                      # per wave
        tot_b = acc[0] + acc[2] + sb + rb + fb
        tot_e = acc[1] + acc[3] + se + re_ + fe
        out.append((new, acc, (sb, se), (rb, re_), (fb, fe), tot_e / (tot_b + tot_e)))
    print(f"{kind}-major kernel, QPW = {qpw}, QPB = {qpb}   (LDS-array cycles per wave: base + extra from conflicts)")
    for new, acc, st, rs, fr, share in out:
        print(f"  {'new' if new else 'old'}: cell reads {acc[0]:.0f} + {acc[1]:.2f}   axis reads {acc[2]:.0f} + {acc[3]:.2f}   staging stores {st[0]} + {st[1]}   "
              f"result stores {rs[0]} + {rs[1]}   final reads {fr[0]:.1f} + {fr[1]:.1f}   conflict share {100 * share:.1f} %")
    return out


def main() -> int:
    res = [report("row", 2, 16), report("row", 4, 32), report("tiled", 2, 16), report("tiled", 4, 32)]
    # what the source comments claim: the row-major tap phase and its result stores are conflict-free, and nothing got worse
    ok = True
    for (old, new) in ((r[0], r[1]) for r in res[:2]):
        ok &= new[1][1] == 0 and new[1][3] == 0 and new[3][1] == 0 and new[2][1] <= old[2][1] and new[4][1] <= old[4][1]
    for (old, new) in ((r[0], r[1]) for r in res[2:]):
        ok &= new[1][1] < old[1][1] and new[2][1] <= old[2][1]
    print("claims hold" if ok else "CLAIMS VIOLATED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
