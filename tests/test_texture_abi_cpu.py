"""CPU: the staged texture group.  Its header lies in eonerf_code_amd/csrc/ (eonerf_texture.h) and its bindings in
_lib.API_STAGED_TEXTURE until a follow-up moves both beside the public ones; this test holds that table to the header's prototypes with
the public test's own reader (tests/test_library_abi.py: declarations, agrees), the staged names apart from every public and every
other staged one, and the header's constants to the restatement's."""
import ctypes
import os

from conftest import REPO
from test_library_abi import agrees, declarations

STAGED = os.path.join(REPO, "eonerf_code_amd", "csrc")
PROTOTYPES = {"eonerf_texture.h": 5}


def test_staged_table_agrees_with_the_staged_header():
    from eonerf_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert set(_lib.API_STAGED_TEXTURE) == set(PROTOTYPES)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for header, table in _lib.API_STAGED_TEXTURE.items():
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
    older = (_lib.API_STAGED, _lib.API_STAGED_SMOOTH, _lib.API_STAGED_RAYCAST)
    tables = list(_lib.API.values()) + [group for staged in older for group in staged.values()]
    other = {name for group in tables for name in group}
    for header in _lib.API:
        other |= set(declarations(header)[0])
    for staged in older:
        for header in staged:
            other |= set(declarations(os.path.join(STAGED, header))[0])
    staged = [name for group in _lib.API_STAGED_TEXTURE.values() for name in group]
    assert len(staged) == len(set(staged)) and not other & set(staged)
    assert not (set(_lib.API) | set(_lib.API_STAGED) | set(_lib.API_STAGED_SMOOTH) | set(_lib.API_STAGED_RAYCAST)) & set(_lib.API_STAGED_TEXTURE)


def test_the_header_says_it_is_staged_and_its_constants_are_the_restatement_s():
    import ortho_restated as orr
    import texture_restated as tr
    text = open(os.path.join(STAGED, "eonerf_texture.h")).read()
    assert "STAGED" in text.split("\n")[0]
    for name, value in (("VERSION", tr.VERSION), ("MAX_TEXELS", tr.MAX_TEXELS), ("GUTTER", tr.GUTTER), ("MAX_SIDE", tr.MAX_SIDE),
                        ("MAX_MEDIAN", tr.MAX_MEDIAN), ("MEAN", tr.MEAN), ("MEDIAN", tr.MEDIAN), ("BEST", tr.BEST)):
        assert f"#define EONERF_TEXTURE_{name} {value} " in text or f"#define EONERF_TEXTURE_{name} {value}\n" in text, name
    # the two modes the bake shares with eonerf_ortho_fuse carry the same numbers, and the median the same limit
    assert (tr.MEAN, tr.MEDIAN, tr.MAX_MEDIAN) == (orr.MEAN, orr.MEDIAN, orr.MAX_MEDIAN)
    from eonerf_code_amd import texture
    assert texture.MAX_TEXELS == tr.MAX_TEXELS and texture.MAX_MEDIAN == tr.MAX_MEDIAN
    assert texture._MODES == {"mean": tr.MEAN, "median": tr.MEDIAN, "best": tr.BEST}
