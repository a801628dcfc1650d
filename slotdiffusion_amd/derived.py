"""Derived weight operands that are re-made once per optimiser step inside the captured step.

A family of such operands (dgrad operands, e4m3fn operands, the unit streams of the fused SpatialTransformer training
kernels) keeps its members in persistent buffers and re-makes ALL of them with one launch over a descriptor table that
lives on the device.  `StepTable` owns what the families share: members in registration order, the epoch / stale
bookkeeping, the cached device table per group, the one host-to-device copy (refused inside a graph capture) and the
check that the arenas the descriptors point into are still the model's.  A family supplies how a member's descriptors
are filled and how a table / a first use is launched -- nothing else.
"""
import types

import numpy as np
import torch

from . import _lib


def put(rows, i, **fields):
    """Set fields of descriptor `i` of a table (numpy records of a C ABI struct) by name."""
    for k, v in fields.items():
        rows[k][i] = v


def table_tensor(arr, device):
    """Descriptor records -> their bytes as a uint8 tensor on `device` (THE host-to-device copy of a table)."""
    return torch.from_numpy(arr.view(np.uint8)).to(device)


class StepTable:
    """fill(member, rows, block_begin) -> next block_begin   writes the member's `member.rows` descriptors
    launch(group, table)                                     the grouped launch: table.dev (uint8 tensor on the device),
                                                             table.rows descriptors, table.blocks workgroups
    first(member, one)                                       the member's first use; one() -> its own table (a copy)
    sources() -> tuple                                       base pointers the descriptors point into"""

    def __init__(self, family, struct, fill, launch, first, sources,
                 capturing=torch.cuda.is_current_stream_capturing):
        self.family = family
        self.desc = np.dtype(_lib.CSTRUCT[struct])
        self._fill, self._launch, self._first, self._sources, self._capturing = fill, launch, first, sources, capturing
        self.members = {}            # key -> record, in registration order
        self.epoch, self.stale = 0, False
        self.uploads = 0             # host -> device table copies so far
        self._tables = {}            # group -> device table, dropped when the group gains a member
        self._built = None           # sources() at the first registration: what every descriptor points into

    def mark_stale(self):
        self.stale = True

    def get(self, key):
        """The member if it was made from the current weights, else None (the caller registers it)."""
        if self.stale:
            self.refresh()
        m = self.members.get(key)
        return m if m is not None and m.epoch == self.epoch else None

    def add(self, key, m, device, group=None, rows=1, tabled=True):
        """Make member `m` now (its first use) and register it.  tabled=False: not part of the grouped launch -- it is
        current for this epoch only and comes back here."""
        if not self.members:
            self._built = self._sources()
        m.key, m.group, m.rows, m.tabled, m.device = key, group, rows, tabled, device

        def one():
            m.first_table = self._upload([m])         # (kept alive past the launch)
            return m.first_table
        self._first(m, one)
        m.epoch = self.epoch
        self.members[key] = m
        if tabled:
            self._tables.pop(group, None)
        return m

    def refresh(self):
        """Re-make every tabled member: one launch per group, over the cached table unless the group gained a member."""
        if self._sources() != self._built:
            # the arenas were re-created: every descriptor points into freed memory.  Nothing is launched; the members
            # register afresh at their next request
            self.members.clear()
            self._tables.clear()
            self.stale = False
            return
        self.epoch += 1
        groups = {}
        for m in self.members.values():
            if m.tabled:
                groups.setdefault(m.group, []).append(m)
        for group, ms in groups.items():
            tab = self._tables.get(group)
            if tab is None:
                tab = self._tables[group] = self._upload(ms)
            self._launch(group, tab)
            for m in ms:
                m.epoch = self.epoch
        self.stale = False

    def _upload(self, ms):
        if self._capturing():
            raise _lib.SdmiError(f'{self.family} {ms[-1].key}: its descriptor table is a host-to-device copy, which a '
                                 'graph capture cannot hold (first use, or first re-make after it was registered): '
                                 'run the warm-up passes before capturing')
        arr = np.zeros(sum(m.rows for m in ms), dtype=self.desc)
        o = blk = 0
        for m in ms:
            blk = self._fill(m, arr[o:o + m.rows], blk)
            o += m.rows
        self.uploads += 1
        return types.SimpleNamespace(dev=table_tensor(arr, ms[0].device), rows=len(arr), blocks=blk)

