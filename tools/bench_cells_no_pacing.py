#!/usr/bin/env python3
"""bench.py with OXHIP_DEBUG_CELLS_NO_PACING set on every batch it creates: the frozen cell-grid launches report their progress
to the board as always, but no wave changes its issue priority.  Against a plain bench.py run of the same build this separates
what the reports cost from what the priorities gain (profiles/frozen_pacing/).
usage: bench_cells_no_pacing.py <bench.py's arguments>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oxmpl_amd import capi  # noqa: E402

_init = capi.RRTBatch.__init__


def _init_no_pacing(self, *args, **kw):
    names = _init.__code__.co_varnames[1:_init.__code__.co_argcount]
    at = names.index("debug_flags")
    if len(args) > at:
        args = args[:at] + (args[at] | capi.DEBUG_CELLS_NO_PACING,) + args[at + 1:]
    else:
        kw["debug_flags"] = kw.get("debug_flags", 0) | capi.DEBUG_CELLS_NO_PACING
    _init(self, *args, **kw)


capi.RRTBatch.__init__ = _init_no_pacing
import bench  # noqa: E402

bench.main()
