"""CPU: the staged dual-contouring group.  Its header lies in eonerf_code_amd/csrc/ (eonerf_dual.h) and its bindings in
_lib.API_STAGED_DUAL until a follow-up moves both beside the public ones; this test holds that table to the header's prototypes with
the public test's own reader (tests/test_library_abi.py: declarations, agrees), the staged names apart from every public and every
other staged one, and the header's constants to the restatement's."""
import ctypes
import os
import re

from conftest import REPO
from test_library_abi import agrees, declarations

STAGED = os.path.join(REPO, "eonerf_code_amd", "csrc")
PROTOTYPES = {"eonerf_dual.h": 5}


def test_staged_table_agrees_with_the_staged_header():
    from eonerf_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert set(_lib.API_STAGED_DUAL) == set(PROTOTYPES)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for header, table in _lib.API_STAGED_DUAL.items():
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
    assert L.eonerf_dual_version() == 1                       # (a host function: no device is touched)


def test_staged_names_collide_with_nothing_public_or_staged():
    from eonerf_code_amd import _lib
    older = (_lib.API_STAGED, _lib.API_STAGED_SMOOTH, _lib.API_STAGED_RAYCAST, _lib.API_STAGED_TEXTURE)
    tables = list(_lib.API.values()) + [group for staged in older for group in staged.values()]
    other = {name for group in tables for name in group}
    for header in _lib.API:
        other |= set(declarations(header)[0])
    for staged in older:
        for header in staged:
            other |= set(declarations(os.path.join(STAGED, header))[0])
    staged = [name for group in _lib.API_STAGED_DUAL.values() for name in group]
    assert len(staged) == len(set(staged)) == 5 and not other & set(staged)
    assert not (set(_lib.API) | {header for table in older for header in table}) & set(_lib.API_STAGED_DUAL)


def test_the_header_says_it_is_staged_and_its_constants_are_the_restatement_s():
    import dual_cases as dc
    import dual_restated as dr
    text = open(os.path.join(STAGED, "eonerf_dual.h")).read()
    assert "STAGED" in text.split("\n")[0]

    def constant(name, source=text):
        return int(re.search(rf"#define\s+{name}\s+(-?\d+)\s", source).group(1))
    assert constant("EONERF_DUAL_VERSION") == dr.VERSION and constant("EONERF_DUAL_STATUS_CAPACITY") == dr.STATUS_CAPACITY
    assert 2.0 ** constant("EONERF_DUAL_MIN_REG_LOG2") == dr.MIN_REGULARISATION and 2.0 ** constant("EONERF_DUAL_MAX_REG_LOG2") == dr.MAX_REGULARISATION
    assert constant("EONERF_MESH_TILE", open(os.path.join(REPO, "include", "eonerf_mesh.h")).read()) == dc.TILE
    from eonerf_code_amd import mesh
    assert (mesh.DUAL_MIN_REGULARISATION, mesh.DUAL_MAX_REGULARISATION) == (dr.MIN_REGULARISATION, dr.MAX_REGULARISATION)
    assert mesh.STATUS_CAPACITY == dr.STATUS_CAPACITY and mesh.DUAL_REGULARISATION == 0.1 and mesh.MESH_METHODS == ("tetra", "dual")
