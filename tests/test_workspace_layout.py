"""Every workspace is described once, by a layout function (sn::Carver, sparenet_amd/csrc/common.hpp) that the size
export measures and the entry point carves.  The size exports are pure host code, so this runs without a GPU: what
they return -- and where sn_emd_diag_offset puts the diagnostic words -- must stay what the build before the layout
functions returned, over a grid that crosses every branch (tools/record_workspace_sizes.py wrote the table)."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")


def _declared_size_exports():
    hdr = open(os.path.join(ROOT, "include", "sparenet_hip.h")).read()
    return sorted(set(re.findall(r"^size_t\s+(sn_[a-z0-9_]+)\s*\(", hdr, re.M)))


def test_every_size_export_has_recorded_rows():
    """A size export declared in the header without rows in the table fails here: the next op cannot skip the check."""
    table = json.load(open(TABLE))
    names = _declared_size_exports()
    assert "sn_emd_diag_offset" in names, names
    assert all(n.endswith("_workspace_bytes") or n == "sn_emd_diag_offset" for n in names), names
    for n in names:
        rows = table.get(n)
        assert rows, f"{n} is declared in include/sparenet_hip.h but tests/golden/workspace_sizes.json has no rows for it"
        assert any(r[-1] > 0 for r in rows), f"{n}: no valid shape recorded"
        if n != "sn_emd_diag_offset":
            assert any(r[-1] == 0 and min(r[:-1]) < 1 for r in rows), f"{n}: no invalid shape recorded"
    assert sorted(table) == names, "rows of an export the header no longer declares"


def test_size_exports_return_the_recorded_sizes():
    import sparenet_amd

    lib = sparenet_amd.lib()
    table = json.load(open(TABLE))
    bad = []
    for name, rows in table.items():
        fn = getattr(lib, name)
        for *args, want in rows:
            got = fn(*args)
            if got != want:
                bad.append(f"{name}{tuple(args)} = {got}, recorded {want}")
    assert not bad, "\n".join(bad[:40])
