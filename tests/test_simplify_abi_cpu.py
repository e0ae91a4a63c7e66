"""CPU: the staged simplification group.  Its header lies in eonerf_code_amd/csrc/ (eonerf_simplify.h) and its bindings in
_lib.API_STAGED until a follow-up moves both beside the public ones; this test holds that table to the header's prototypes with the
public test's own reader (tests/test_library_abi.py: declarations, agrees), and the staged names apart from every public one."""
import ctypes
import os

from conftest import REPO
from test_library_abi import agrees, declarations

STAGED = os.path.join(REPO, "eonerf_code_amd", "csrc")
PROTOTYPES = {"eonerf_simplify.h": 4}


def test_staged_table_agrees_with_the_staged_header():
    from eonerf_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert set(_lib.API_STAGED) == set(PROTOTYPES)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for header, table in _lib.API_STAGED.items():
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


def test_staged_names_collide_with_nothing_public():
    from eonerf_code_amd import _lib
    public = {name for group in _lib.API.values() for name in group}
    for header in _lib.API:
        public |= set(declarations(header)[0])
    staged = [name for group in _lib.API_STAGED.values() for name in group]
    assert len(staged) == len(set(staged)) and not public & set(staged)
    assert not set(_lib.API) & set(_lib.API_STAGED)


def test_the_header_says_it_is_staged_and_its_constants_are_the_restatement_s():
    import simplify_restated as sr
    text = open(os.path.join(STAGED, "eonerf_simplify.h")).read()
    assert "STAGED" in text.split("\n")[0]
    for name, value in (("SUBCELL_BITS", sr.SUBCELL_BITS), ("MAX_DIM", sr.MAX_DIM), ("MEAN", sr.MEAN), ("NEAREST", sr.NEAREST)):
        assert f"#define EONERF_SIMPLIFY_{name} {value}\n" in text, name
    assert "#define EONERF_SIMPLIFY_MAX_CELLS (1 << 27)\n" in text and sr.MAX_CELLS == 1 << 27
