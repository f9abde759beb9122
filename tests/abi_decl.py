"""Shared by the CPU tests of the C ABI (tests/test_decode_abi.py, test_decode_paged_abi.py, test_decode_fp8_abi.py, test_gqa_abi.py):
what include/flash_attention.h declares, and host memory that passes the pointer checks so that a call stops at the argument under
test -- no GPU is touched."""
import ctypes
import os
import re

import __graft_entry__ as entry


def declared_parameters(name):
    """the parameter names of `name` as include/flash_attention.h declares it"""
    text = open(os.path.join(entry.ROOT, "include", "flash_attention.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, name
    return [re.sub(r"[\s*]+", " ", a).split()[-1] for a in m.group(1).split(",")]


def aligned_host_pointer():
    """(buffer, a 16-byte aligned address inside it): keep the buffer alive as long as the address is used"""
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 15) & ~15
