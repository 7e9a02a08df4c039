"""``ops.ClockStamps.ghz()`` pairs two stamps CU by CU (the measurement behind it: profiles/clock_stamp_per_cu.txt): the counters
of two CUs of one XCD need not share an origin, and two launches need not land on the same CUs.  No GPU: the stamp records --
word 0 the place (XCD in bits 3:0, CU in bits 11:4), word 1 the shader-clock counter, word 2 the 100 MHz counter -- are
written by hand."""

import torch


def _place(xcd, se, cu):
    return xcd | (se << 5 | cu) << 4            # HW_ID bits 15:8 above the XCD id: CU 3:0, array 4, shader engine 7:5


def _stamps(capacity=2):
    from vdpp_amd.hip import ops
    return ops.ClockStamps(torch.device("cpu"), capacity)


def _write(st, slot, places, real, ghz, origin):
    """One stamp at 100 MHz tick ``real``: workgroup ``i`` ran on ``places[i % len(places)]``, whose counter started at
    ``origin[place]`` and ticks at ``ghz`` (a number, or place -> number)."""
    for i in range(st.BLOCKS):
        p = places[i % len(places)]
        rate = ghz[p] if isinstance(ghz, dict) else ghz
        st.buf[slot, i, 0] = p
        st.buf[slot, i, 1] = origin[p] + int(real * rate * 10)
        st.buf[slot, i, 2] = 7000 + real
        st.buf[slot, i, 3] = 1
    st.n = max(st.n, slot + 1)


CUS = [_place(x, se, cu) for x in (0, 3) for se in range(4) for cu in range(8)]
ORIGIN = {p: 10**11 * (p & 15) + 3 * 10**8 * (i % 7) + 12345 * i for i, p in enumerate(CUS)}   # 3e8 ticks apart within an XCD


def test_cus_of_one_xcd_with_unrelated_origins_in_another_order():
    """64 CUs of two XCDs, every CU's counter with its own origin; the last stamp's workgroups land on the CUs in another order.
    Pairing the first workgroup of an XCD with the first of that XCD (as before CUs were noted) would be off by the origins."""
    st = _stamps()
    _write(st, 0, CUS, 0, 1.9, ORIGIN)
    _write(st, 1, CUS[5:] + CUS[:5], 2_000_000, 1.9, ORIGIN)
    ghz, secs, xcds = st.ghz()
    assert xcds == 2 and abs(ghz - 1.9) < 1e-6 and abs(secs - 0.02) < 1e-9
    # the same records paired XCD by XCD: what the CU bits are for
    first, last = st.buf[0], st.buf[1]
    old = [0.1 * int(last[(last[:, 0] & 15) == x][0][1] - first[(first[:, 0] & 15) == x][0][1]) / 2_000_000 for x in (0, 3)]
    assert max(abs(r - 1.9) for r in old) > 1.0, old


def test_only_cus_seen_in_both_stamps_are_paired():
    st = _stamps()
    _write(st, 0, CUS[:40], 0, 2.1, ORIGIN)               # XCD 0 whole, XCD 3's first 8 CUs
    _write(st, 1, CUS[36:], 1_000_000, 2.1, ORIGIN)       # XCD 3 whole: 4 CUs in both stamps, all on XCD 3
    ghz, secs, xcds = st.ghz()
    assert xcds == 1 and abs(ghz - 2.1) < 1e-6 and abs(secs - 0.01) < 1e-9
    st = _stamps()
    _write(st, 0, CUS[:32], 0, 2.1, ORIGIN)
    _write(st, 1, CUS[32:], 1_000_000, 2.1, ORIGIN)
    assert st.ghz() is None                               # no CU in both: nothing to pair, not a guess


def test_each_xcd_gives_its_median_cu():
    """A CU whose counter stood still for part of the stretch (or jumped) does not move its XCD's figure; XCDs at different
    clocks are averaged."""
    st = _stamps()
    rate = {p: (1.8 if p & 15 == 0 else 2.2) for p in CUS}
    rate[CUS[3]], rate[CUS[40]] = 0.4, 9.0
    _write(st, 0, CUS, 0, rate, ORIGIN)
    _write(st, 1, CUS, 2_000_000, rate, ORIGIN)
    ghz, secs, xcds = st.ghz()
    assert xcds == 2 and abs(ghz - 2.0) < 1e-6


def test_first_and_last_of_several_stamps_in_any_slot():
    st = _stamps(3)
    _write(st, 2, CUS, 0, 1.7, ORIGIN)
    _write(st, 0, CUS, 500_000, 1.7, ORIGIN)
    _write(st, 1, CUS[::-1], 3_000_000, 1.7, ORIGIN)
    ghz, secs, xcds = st.ghz()
    assert xcds == 2 and abs(ghz - 1.7) < 1e-6 and abs(secs - 0.03) < 1e-9
