"""Host-side checks of the batch-tiled loss step (carel_tail_losses_tiled, carel_tail_batch_limit): the limit table of
carel_tail_losses from the library's own LDS plans, the new symbols against the header and the binding, the refusals that need no
device, and the workspace layout (regions are only appended: the pair_dead flag that carel_adam_step points at stays where it was).
No GPU: nothing here reaches a HIP call."""
import ctypes as C
import os
import re

from carel_vae_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2


def test_batch_limit_is_the_table_of_the_header():
    lib = L.load()
    assert [lib.carel_tail_batch_limit(D, 6) for D in (8, 16, 24, 32)] == [142, 127, 114, 101]
    assert [lib.carel_tail_batch_limit(24, EC) for EC in (1, 6, 8)] == [114, 114, 114]          # the decoder binds there
    assert [lib.carel_tail_batch_limit(D, EC) for D, EC in ((0, 6), (33, 6), (24, 0), (24, 9))] == [0, 0, 0, 0]


def test_header_and_binding_declare_both_functions():
    text = open(os.path.join(ROOT, "include", "carel_hip.h")).read()
    assert re.search(r"\bint32_t\s+carel_tail_batch_limit\s*\(\s*int32_t\s+ec_dim\s*,\s*int32_t\s+e_classes\s*\)\s*;", text)
    assert re.search(r"\bint\s+carel_tail_losses_tiled\s*\(\s*const\s+carel_tail_args\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", text)
    assert L.SIGNATURES["carel_tail_batch_limit"] == (C.c_int32, [C.c_int32, C.c_int32])
    assert L.SIGNATURES["carel_tail_losses_tiled"] == L.SIGNATURES["carel_tail_losses"]
    lib = L.load()
    assert lib.carel_abi_version() == 9 == L.ABI_VERSION


def test_null_args_and_oversize_batch_are_refused_on_the_host():
    lib = L.load()
    assert lib.carel_tail_losses_tiled(None, None) == ERR_ARG
    a = L.TailArgs()                      # zeroed: every pointer NULL, so anything past the batch check would be an argument error
    a.batch, a.seq_len, a.hidden, a.ec_dim, a.e_classes, a.bow_dim = 1025, 32, 768, 24, 6, 257
    assert lib.carel_tail_losses_tiled(C.byref(a), None) == ERR_SHAPE
    msg = lib.carel_last_error().decode()
    assert "carel_tail_losses_tiled" in msg and "1024" in msg, msg
    a.batch = 1024
    assert lib.carel_tail_losses_tiled(C.byref(a), None) == ERR_ARG          # (NULL tensors, found before any HIP call)


def test_workspace_only_grows_by_appended_regions():
    lib = L.load()
    # carel_tail_workspace_floats / carel_tail_pair_dead_offset at the benchmark's shape before the tiled form existed
    assert lib.carel_tail_workspace_floats(64, 24, 23771) >= 1945152
    assert lib.carel_tail_pair_dead_offset(64, 24, 23771) == 1937920
