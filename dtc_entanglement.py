#!/usr/bin/env python3
"""Reduced density matrices of site windows, their entropy and purity on the
MI355X engine (no reference counterpart; flags as dtc_autocorr.py /
dtc_energy.py).  See <package>/entanglement_cli.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from __graft_entry__ import load_package  # noqa: E402

if __name__ == "__main__":
    raise SystemExit(load_package().entanglement_cli.main())
