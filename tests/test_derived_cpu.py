"""CPU-side checks of derived.StepTable (the per-step derived weight operands) with the three real
descriptor structs and WeightBank's own fill / launch callbacks (wired as WeightBank.__init__ wires them): CPU tensors stand for the operands, `kern.call` is
replaced by a recorder and the capture predicate is injected.  No kernel is launched here."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from slotdiffusion_amd import _lib, derived, kern

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture
def bank(monkeypatch):
    """A WeightBank reduced to its three step tables -> (bank, recorded calls, state to steer capture / sources)."""
    calls = []
    monkeypatch.setattr(kern, 'call', lambda fname, stream, **kw: calls.append((fname, kw)))
    monkeypatch.setattr(kern, '_st', lambda: 0)
    state = SimpleNamespace(capturing=False, src=(0x1000, 0x2000))
    wb = kern.WeightBank.__new__(kern.WeightBank)
    wb._q_amax, wb._q_inv = torch.zeros(8, dtype=torch.int32), torch.zeros(8)

    def table(family, struct, fill, launch, first):
        return derived.StepTable(family, struct, fill, launch, first, lambda: state.src, capturing=lambda: state.capturing)
    wb.dgrad_ops = table('dgrad operand', 'SdmiPackDesc', wb._dgrad_fill, wb._dgrad_launch, wb._dgrad_first)
    wb.fp8_ops = table('fp8 operand', 'SdmiFp8Desc', wb._fp8_fill, wb._fp8_launch,
                       lambda m, one: wb._fp8_launch(None, one(), m.slot))
    wb.st_streams = table('fused training block', 'SdmiStPackDesc', wb._st_fill, wb._st_launch,
                          lambda m, one: wb._st_launch(None, one()))
    return wb, calls, state


# ---- members and, filled independently of the code under test, the tables they must give ----------------------------
_SHAPES = [(3, 3, 3, 128), (64, 3, 3, 64), (200, 1, 1, 136), (72, 4, 4, 8)]       # Cout, KH, KW, Cin


def _dgrad_member(i, dtype=BF16, sub=None):
    co, kh, kw, ci = _SHAPES[i % len(_SHAPES)]
    npad = (co + 7) // 8 * 8
    taps = kh * kw if sub is None else sub[3] * sub[4]
    return SimpleNamespace(dst=torch.empty(ci * taps, npad, dtype=dtype), src=torch.empty(co, kh * kw * ci, dtype=dtype),
                           Cout=co, KH=kh, KW=kw, Cin=ci, CoutPad=npad, sub=sub)


def _dgrad_expect(ms):
    arr = (_lib.CSTRUCT['SdmiPackDesc'] * len(ms))()
    blk = 0
    for d, m in zip(arr, ms):
        d.src, d.dst = m.src.data_ptr(), m.dst.data_ptr()
        d.Cout, d.KH, d.KW, d.Cin, d.CoutPad, d.block_begin = m.Cout, m.KH, m.KW, m.Cin, m.CoutPad, blk
        taps = m.KH * m.KW
        if m.sub is not None:
            d.kh0, d.kw0, d.kstep, d.nkh, d.nkw = m.sub
            taps = m.sub[3] * m.sub[4]
        blk += taps * ((m.Cout + 63) // 64) * ((m.Cin + 63) // 64)
    return bytes(arr), blk


def _fp8_member(wb, i):
    src = torch.empty(16 * (300 + 77 * i), 16)
    return SimpleNamespace(q=torch.empty(src.shape, dtype=torch.uint8), inv=wb._q_inv[i:i + 1], src=src, slot=i)


def _fp8_expect(ms):
    arr = (_lib.CSTRUCT['SdmiFp8Desc'] * len(ms))()
    blk = 0
    for d, m in zip(arr, ms):
        d.src, d.dst, d.n, d.block_begin = m.src.data_ptr(), m.q.data_ptr(), m.src.numel(), blk
        blk += (m.src.numel() + 4095) // 4096
    return bytes(arr), blk


def _st_member(wb, C):
    """What WeightBank.st_train_streams registers, on CPU tensors."""
    shapes = dict(po=(C, C), ff2=(C, 4 * C), ff1=(8 * C, C), o2=(C, C), q2=(C, C), o=(C, C), q=(C, C), k=(C, C), v=(C, C))
    shapes['in'] = (C, C)
    mats = {k: torch.empty(sh, dtype=BF16) for k, sh in shapes.items()}
    units = kern.st_train_units(C)
    count = {k: sum(len(w) for w in units[k]) for k in wb.ST_STREAMS}
    st = {'w' + k: torch.empty(count[k] * 1024, dtype=BF16) for k in wb.ST_STREAMS}
    descs = np.zeros(sum(count.values()), dtype=wb.st_streams.desc)
    o = 0
    for k in wb.ST_STREAMS:
        kern.st_pack_descs(descs[o:o + count[k]], units[k], mats, st['w' + k])
        o += count[k]
    return SimpleNamespace(streams=dict(st, C=C), descs=descs, mats=mats, units=units)


def _st_expect(ms):
    arr = (_lib.CSTRUCT['SdmiStPackDesc'] * sum(len(m.descs) for m in ms))()
    i = 0
    for m in ms:
        for k in kern.WeightBank.ST_STREAMS:
            base = m.streams['w' + k].data_ptr()
            for j, (key, r0, k0, tr) in enumerate(u for wave in m.units[k] for u in wave):
                w = m.mats[key]
                ld = w.shape[1]
                d = arr[i]
                d.dst = base + 2048 * j
                if tr:
                    d.src, d.rs, d.cs = w.data_ptr() + 2 * (k0 * ld + r0), 1, ld
                else:
                    d.src, d.rs, d.cs = w.data_ptr() + 2 * (r0 * ld + k0), ld, 1
                i += 1
    return bytes(arr), 0


class Fam:
    def __init__(self, wb, name):
        self.name = name
        self.table = dict(dgrad=wb.dgrad_ops, fp8=wb.fp8_ops, st=wb.st_streams)[name]
        self.entry = dict(dgrad='sdmi_pack_dgrad_batch', fp8='sdmi_fp8_quant_group', st='sdmi_st_pack')[name]
        self.count = 'n_units' if name == 'st' else 'n_desc'
        self.expect = dict(dgrad=_dgrad_expect, fp8=_fp8_expect, st=_st_expect)[name]
        self.wb = wb

    def add(self, i):
        if self.name == 'dgrad':       # a parity sub-filter: its first use needs a table, like the other families'
            m = _dgrad_member(i, sub=(i % 2, 1, 2, 2 - i % 2, 1))
            return self.table.add(('sub', i), m, 'cpu', group=BF16)
        if self.name == 'fp8':
            return self.table.add(f'w{i}', _fp8_member(self.wb, i), 'cpu')
        m = _st_member(self.wb, 128)
        return self.table.add(f'block{i}', m, 'cpu', rows=len(m.descs))

    def check(self, call, ms):
        """A recorded table launch carries exactly the descriptors of `ms`, in this order."""
        fname, kw = call
        want, blocks = self.expect(ms)
        assert fname == self.entry and kw[self.count] * self.table.desc.itemsize == len(want)
        assert ctypes.string_at(kw['descs'], len(want)) == want
        if self.name != 'st':
            assert kw['total_blocks'] == blocks


FAMILIES = ('dgrad', 'fp8', 'st')


@pytest.mark.parametrize('name', FAMILIES)
def test_registration_is_one_single_entry_launch_and_a_second_get_none(bank, name):
    wb, calls, _ = bank
    fam = Fam(wb, name)
    for i in range(3):
        m = fam.add(i)
        assert len(calls) == i + 1
        fam.check(calls[-1], [m])
        if name == 'fp8':             # the one-entry call works on the member's own slot
            assert calls[-1][1]['amax_bits'] == wb._q_amax.data_ptr() + 4 * i
            assert calls[-1][1]['inv_scale'] == wb._q_inv.data_ptr() + 4 * i == m.inv.data_ptr()
    assert list(fam.table.members) == [m.key for m in fam.table.members.values()] and len(fam.table.members) == 3
    for key, m in fam.table.members.items():
        assert fam.table.get(key) is m
    assert len(calls) == 3 and fam.table.uploads == 3


@pytest.mark.parametrize('name', FAMILIES)
def test_stale_table_is_one_grouped_launch_in_registration_order(bank, name):
    wb, calls, _ = bank
    fam = Fam(wb, name)
    ms = [fam.add(i) for i in range(3)]
    del calls[:]
    fam.table.mark_stale()
    assert fam.table.get(ms[1].key) is ms[1]
    assert len(calls) == 1
    fam.check(calls[0], ms)                                   # block_begin = running sum, registration order
    rows = np.frombuffer(ctypes.string_at(calls[0][1]['descs'], calls[0][1][fam.count] * fam.table.desc.itemsize),
                         dtype=fam.table.desc)
    if name == 'fp8':                                         # descriptor i = slot i of the amax / inv-scale buffers
        assert calls[0][1]['amax_bits'] == wb._q_amax.data_ptr() and calls[0][1]['inv_scale'] == wb._q_inv.data_ptr()
        assert [int(r['dst']) for r in rows] == [m.q.data_ptr() for m in sorted(ms, key=lambda m: m.slot)]
        assert [m.slot for m in ms] == [0, 1, 2]
    if name != 'st':
        begins = [int(r['block_begin']) for r in rows]
        assert begins[0] == 0 and begins == sorted(begins) and len(set(begins)) == 3
    for m in ms:                                              # every later request this step launches nothing
        assert fam.table.get(m.key) is m
    assert len(calls) == 1


def test_two_dtypes_are_two_launches_each_over_its_own_members(bank):
    wb, calls, _ = bank
    t = wb.dgrad_ops
    ms = [t.add(i, _dgrad_member(i, dt), 'cpu', group=dt) for i, dt in enumerate((BF16, F32, BF16, F32, BF16))]
    assert [c[0] for c in calls] == ['sdmi_pack_dgrad'] * 5 and t.uploads == 0     # full operands: no table at first use
    del calls[:]
    t.mark_stale()
    assert t.get(3) is ms[3]
    assert len(calls) == 2 and t.uploads == 2
    fam = Fam(wb, 'dgrad')
    for call, dt in zip(calls, (BF16, F32)):
        fam.check(call, [m for m in ms if m.group == dt])
        assert call[1]['dtype'] == kern._DT[dt]


def test_member_outside_the_table_comes_back_every_epoch(bank):
    """A dgrad operand whose source is a materialised copy: never in the grouped launch, current for one epoch."""
    wb, calls, _ = bank
    t = wb.dgrad_ops
    a = t.add('a', _dgrad_member(0), 'cpu', group=BF16)
    b = t.add('b', _dgrad_member(1), 'cpu', group=BF16, tabled=False)
    del calls[:]
    t.mark_stale()
    assert t.get('b') is None and t.members['b'] is b and t.get('a') is a
    assert len(calls) == 1
    Fam(wb, 'dgrad').check(calls[0], [a])


@pytest.mark.parametrize('name', FAMILIES)
def test_table_is_rebuilt_only_after_an_addition(bank, name):
    wb, calls, _ = bank
    fam = Fam(wb, name)
    ms = [fam.add(i) for i in range(2)]
    fam.table.mark_stale()
    fam.table.get(ms[0].key)
    up, first = fam.table.uploads, calls[-1][1]['descs']
    fam.table.mark_stale()
    fam.table.get(ms[0].key)
    assert fam.table.uploads == up and calls[-1][1]['descs'] == first      # the same device table, no new copy
    ms.append(fam.add(2))
    assert fam.table.uploads == up + 1                                      # (its own one-entry table)
    del calls[:]
    fam.table.mark_stale()
    assert fam.table.get(ms[2].key) is ms[2]
    assert fam.table.uploads == up + 2 and len(calls) == 1
    fam.check(calls[0], ms)                                                 # n + 1 descriptors


@pytest.mark.parametrize('name', FAMILIES)
def test_host_to_device_copies_are_refused_inside_a_capture(bank, name):
    wb, calls, state = bank
    fam = Fam(wb, name)
    ms = [fam.add(i) for i in range(2)]
    fam.table.mark_stale()
    fam.table.get(ms[0].key)
    state.capturing = True
    n = len(calls)
    fam.table.mark_stale()
    assert fam.table.get(ms[1].key) is ms[1] and len(calls) == n + 1        # a refresh over the existing table: legal
    with pytest.raises(_lib.SdmiError, match=fam.table.family):             # registration: its table is a copy
        fam.add(2)
    assert len(fam.table.members) == 2 and len(calls) == n + 1
    state.capturing = False
    ms.append(fam.add(2))
    state.capturing = True
    fam.table.mark_stale()
    with pytest.raises(_lib.SdmiError, match=re.escape(str(ms[2].key))):
        fam.table.get(ms[0].key)                                            # the rebuild names the new member
    assert len(calls) == n + 2                                              # (nothing launched by the refused refresh)


def test_dgrad_full_operand_first_use_is_legal_inside_a_capture(bank):
    wb, calls, state = bank
    state.capturing = True
    m = wb.dgrad_ops.add('full', _dgrad_member(1), 'cpu', group=BF16)
    assert [c[0] for c in calls] == ['sdmi_pack_dgrad'] and wb.dgrad_ops.get('full') is m and wb.dgrad_ops.uploads == 0
    kw = calls[0][1]
    assert (kw['src'], kw['dst'], kw['Cout'], kw['CoutPad']) == (m.src.data_ptr(), m.dst.data_ptr(), m.Cout, m.CoutPad)


@pytest.mark.parametrize('name', FAMILIES)
def test_changed_sources_drop_the_table_without_launching_it(bank, name):
    wb, calls, state = bank
    fam = Fam(wb, name)
    ms = [fam.add(i) for i in range(2)]
    fam.table.mark_stale()
    fam.table.get(ms[0].key)
    del calls[:]
    state.src = (0x1000, 0x3000)                    # the shadow arena was re-created
    fam.table.mark_stale()
    assert fam.table.get(ms[0].key) is None and fam.table.get(ms[1].key) is None
    assert calls == [] and len(fam.table.members) == 0
    m = fam.add(0)                                  # a new request registers afresh ...
    assert len(calls) == 1 and fam.table.get(m.key) is m
    fam.table.mark_stale()
    assert fam.table.get(m.key) is m                # ... against the new sources
    assert len(calls) == 2
    fam.check(calls[1], [m])


def test_stream_table_layout_comes_from_the_header(bank):
    wb, calls, _ = bank
    assert np.dtype(_lib.CSTRUCT['SdmiStPackDesc']).itemsize == 24 == ctypes.sizeof(_lib.CSTRUCT['SdmiStPackDesc'])
    m = _st_member(wb, 256)
    wb.st_streams.add('block', m, 'cpu', rows=len(m.descs))
    fname, kw = calls[0]
    assert fname == 'sdmi_st_pack' and kw['n_units'] == 2560
    rows = np.frombuffer(ctypes.string_at(kw['descs'], 2560 * 24), dtype=wb.st_streams.desc)
    o = 0
    for k in wb.ST_STREAMS:
        st = m.streams['w' + k]
        n = st.numel() // 1024
        assert [int(d) for d in rows['dst'][o:o + n]] == [st.data_ptr() + 2048 * i for i in range(n)]
        o += n
    assert o == 2560
    assert set(m.streams) == {'wa', 'wb', 'wb1', 'wb2', 'wba', 'C'}


def test_struct_array_fills_by_name_and_rejects_unknown_fields():
    arr = _lib.struct_array('SdmiCopyItem', [dict(src=16, dst=32, bytes=5), dict(dst=64)])
    assert len(arr) == 2 and (arr[0].src, arr[0].dst, arr[0].bytes) == (16, 32, 5) and (arr[1].src, arr[1].dst) == (None, 64)
    with pytest.raises(KeyError):
        _lib.struct_array('SdmiCopyItem', [dict(source=16)])
