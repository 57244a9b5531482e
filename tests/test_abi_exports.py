"""libpt.so exports every function include/pt/pt.h declares.  The runtime is several translation
units linked in one command (path-trace_amd/build_ext.py SOURCES); a file left out of that list would
still link -- a shared library may have undefined references -- and fail only when its entry is called."""
import ctypes
import os
import re

from pathtrace import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pt", "pt.h")


def declared():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    # a declaration: return type, name, '(' -- at the start of a line, outside the comments
    return re.findall(r"^(?:const )?\w+ \*?(pt_\w+)\(", text, flags=re.M)


def test_header_declarations_are_found():
    names = declared()
    assert len(names) == len(set(names)) >= 75, len(names)
    # the parse agrees with the Python binding's own list of the header's functions
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)


def test_every_declared_function_is_exported(built):
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing
