"""The library's stamp covers every source it is built from (CPU; no compiler, no GPU).

``_lib.build()`` rebuilds when ``_lib.source_hash()`` differs from the hash stamped next to the library, so a unit
or header under ``aiocluster_amd/csrc/`` that the hash does not read could change without a rebuild.
"""

import glob
import hashlib
import os

from aiocluster_amd import _lib


def test_every_unit_exists_and_the_core_is_one_of_them():
    assert _lib.UNITS and _lib.SRC in _lib.UNITS
    for path in _lib.UNITS + [_lib.COMMON, _lib.HEADER]:
        assert os.path.isfile(path), path
    assert len(set(_lib.UNITS)) == len(_lib.UNITS)


def test_source_hash_covers_every_file_under_csrc():
    found = sorted(glob.glob(os.path.join(_lib.CSRC, "**", "*.hip"), recursive=True)
                   + glob.glob(os.path.join(_lib.CSRC, "**", "*.h"), recursive=True))
    assert found, "no sources found"
    assert sorted(_lib.UNITS) == [f for f in found if f.endswith(".hip")]  # every unit is built, none listed twice
    missing = [f for f in found if f not in _lib.SOURCES]
    assert not missing, f"not covered by _lib.source_hash(): {missing}"
    assert _lib.HEADER in _lib.SOURCES
    # ... and SOURCES is what the stamp is made of: the flags, then each file's bytes
    h = hashlib.sha256(" ".join(_lib.HIPCC_FLAGS).encode())
    for f in _lib.SOURCES:
        with open(f, "rb") as fh:
            h.update(fh.read())
    assert _lib.source_hash() == h.hexdigest()
