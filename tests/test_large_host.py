"""CPU suite: the C ABI of the large-graph path (vc_large_run) is declared, exported and refuses to run without a device."""
import ctypes as C
import os
import re

import numpy as np

from vechat_amd import capi, large

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vc_large_run", "vc_large_last_error", "vc_large_release")


def _device_visible():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:                                     # noqa: BLE001
        return os.path.exists("/dev/kfd")


def test_large_path_is_declared_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    declared = set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    assert set(NAMES) <= declared
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libvechat_hip.so"))
    assert all(hasattr(lib, n) for n in NAMES)
    assert "VC_WIN_OVERFLOW" in hdr and "vc_large_run" in hdr.split("VC_WIN_OVERFLOW", 1)[1].split("\n", 1)[0]


def _tiny_batch():
    return capi.Batch.from_windows([([b"ACGTACGT", b"ACGTACG", b"CGTACGT"], [b"!" * 8, None, None], [0, 0, 1], [0, 6, 7])], [1])


def test_large_path_without_a_device_is_an_error_not_a_crash(built):
    lib = capi.load_hip()
    # an ordinal no machine has: refused on every box, with or without a GPU
    for dev in ([4096] if _device_visible() else [0, 4096]):
        try:
            large.large_consensus(_tiny_batch(), capi.default_params(device=dev), lib=lib)
        except large.LargeError as e:
            assert e.rc == capi.VC_ERR_NO_DEVICE, str(e)
            assert "device" in lib.vc_large_last_error().decode()
        else:
            raise AssertionError(f"vc_large_run ran on device {dev}")
    large.release(lib)                                    # nothing held: a no-op


def test_large_path_rejects_what_vc_submit_rejects(built):
    if not _device_visible():
        return                                            # (the device check comes first; covered above)
    lib = capi.load_hip()
    b = _tiny_batch()
    bad = capi.Batch(b.win_seq_off, b.seq_off, b.seq_begin, np.array([0, 6, 9], np.uint32), b.seq_has_qual, b.bases, b.quals, b.win_fasta)
    try:
        large.large_consensus(bad, capi.default_params(), lib=lib)
    except large.LargeError as e:
        assert e.rc == capi.VC_ERR_ARG
    else:
        raise AssertionError("a layer ending beyond the backbone was accepted")
