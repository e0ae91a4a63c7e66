"""CPU: the staged ray casting group.  Its header lies in eonerf_code_amd/csrc/ (eonerf_raycast.h) and its bindings in
_lib.API_STAGED_RAYCAST until a follow-up moves both beside the public ones; this test holds that table to the header's prototypes with
the public test's own reader (tests/test_library_abi.py: declarations, agrees), the staged names apart from every public and every
other staged one, and the header's constants to the restatement's."""
import ctypes
import os

from conftest import REPO
from test_library_abi import agrees, declarations

STAGED = os.path.join(REPO, "eonerf_code_amd", "csrc")
PROTOTYPES = {"eonerf_raycast.h": 6}


def test_staged_table_agrees_with_the_staged_header():
    from eonerf_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert set(_lib.API_STAGED_RAYCAST) == set(PROTOTYPES)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for header, table in _lib.API_STAGED_RAYCAST.items():
        assert not os.path.exists(os.path.join(REPO, "include", header)), f"{header} is public now: its table belongs in _lib.API"
        protos, structs = declarations(os.path.join(STAGED, header))            # (an absolute path: the reader joins it to include/)
        assert set(protos) == set(table), set(protos) ^ set(table)
        assert len(protos) == PROTOTYPES[header] and not structs
        for name, (ret, params) in protos.items():
            assert hasattr(L, name), name
            restype, argtypes = table[name]
            assert agrees(ret, restype, named=False), (name, ret, restype)
            assert len(params) == len(argtypes), (name, len(params), len(argtypes))
            for k, (p, t) in enumerate(zip(params, argtypes)):
                assert agrees(p, t), (name, k, p, t)


def test_staged_names_collide_with_nothing_public_or_staged():
    from eonerf_code_amd import _lib
    tables = list(_lib.API.values()) + list(_lib.API_STAGED.values()) + list(_lib.API_STAGED_SMOOTH.values())
    other = {name for group in tables for name in group}
    for header in _lib.API:
        other |= set(declarations(header)[0])
    staged = [name for group in _lib.API_STAGED_RAYCAST.values() for name in group]
    assert len(staged) == len(set(staged)) and not other & set(staged)
    assert not (set(_lib.API) | set(_lib.API_STAGED) | set(_lib.API_STAGED_SMOOTH)) & set(_lib.API_STAGED_RAYCAST)


def test_the_header_says_it_is_staged_and_its_constants_are_the_restatement_s():
    import raycast_restated as rc
    text = open(os.path.join(STAGED, "eonerf_raycast.h")).read()
    assert "STAGED" in text.split("\n")[0]
    for name, value in (("VERSION", rc.VERSION), ("MAX_DIM", rc.MAX_DIM), ("PAD", "0.00390625"), ("TILE", rc.TILE), ("LANE_CELLS", rc.LANE_CELLS),
                        ("MAX_STRIDE", rc.MAX_STRIDE)):
        assert f"#define EONERF_RAYCAST_{name} {value}\n" in text, name
    assert rc.PAD == float("0.00390625") == 2.0 ** -8 and rc.MAX_CELLS == 1 << 27 and rc.MAX_COUNT == (1 << 31) - 1 and rc.MAX_STRIDE == 1 << 24
