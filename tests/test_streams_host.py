"""The stream contract, host side: every entry point of include/gsdeblur.h that takes a stream is either named in the
`covers` of a case of tests/stream_cases.py (the side-stream tests of tests/test_gpu_streams.py then reach it and check
that they did) or listed in its EXEMPT dict with a reason.  A new kernel family cannot be added without deciding."""
import re
from pathlib import Path

import stream_cases as C

HEADER = Path(__file__).resolve().parent.parent / "include" / "gsdeblur.h"


def stream_symbols():
    """every function of the header with a `void* stream` parameter (it is the last one, or — gs_project_fused_bwd_pooled —
    the last but one)"""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    names = []
    for m in re.finditer(r"\b(gs_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        params = [p.strip() for p in m.group(2).split(",")]
        if any(re.fullmatch(r"void\s*\*\s*stream", p) for p in params):
            names.append(m.group(1))
    return names


def test_the_parser_sees_the_header():
    names = stream_symbols()
    assert len(names) == len(set(names)) >= 89
    for known in ("gs_frame_forward", "gs_combine_fwd", "gs_mesh_filter_emit", "gs_project_fused_bwd_pooled", "gs_knn"):
        assert known in names
    assert "gs_version" not in names and "gs_knn_workspace_bytes" not in names


def test_every_entry_point_that_takes_a_stream_is_decided():
    names = set(stream_symbols())
    covered = {s for c in C.CASES for s in c.covers}
    undecided = sorted(names - covered - set(C.EXEMPT))
    assert not undecided, f"neither covered by a case of stream_cases.py nor exempt: {undecided}"
    unknown = sorted((covered | set(C.EXEMPT)) - names)
    assert not unknown, f"not an entry point of gsdeblur.h that takes a stream: {unknown}"
    both = sorted(covered & set(C.EXEMPT))
    assert not both, f"covered AND exempt: {both}"
    for sym, reason in C.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 4, sym


def test_the_table_is_well_formed():
    names = [c.name for c in C.CASES]
    assert len(names) == len(set(names))
    for c in C.CASES:
        assert c.covers and len(c.covers) == len(set(c.covers)) and callable(c.run), c.name


def test_the_binding_knows_every_covered_symbol(gs):
    known = set(gs._lib.exported_names())
    for c in C.CASES:
        assert set(c.covers) <= known, (c.name, sorted(set(c.covers) - known))
