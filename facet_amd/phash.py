"""Perceptual hashes of a batch: what the reference stores per image as `phash = str(imagehash.phash(pil_img))`
(processing/batch_processor.py:216, multi_pass.py:449, scorer.py:972) computed by `fe_phash` on the resident batch.

The engine returns the 64 bits as an integer with the first bit of imagehash's row-major bit array in bit 63, so the reference's
string (`ImageHash.__str__`: the bit string read as a binary number, 16 lowercase hex digits, zero-padded) is the integer in hex.
"""
import numpy as np


def to_hex(hashes):
    """uint64 array -> list of 16-digit lowercase hex strings (leading zeros kept)."""
    return [format(int(v), '016x') for v in np.asarray(hashes, dtype=np.uint64).reshape(-1)]


def from_hex(strings):
    """list of hex strings (as stored in the `phash` column) -> uint64 array; utils/duplicate.py:39-41."""
    return np.array([int(s, 16) for s in strings], dtype=np.uint64)


def phash_batch(engine, images, bgr=False):
    """uint8 [n,h,w,3] RGB images (host array, or the `(ptr, n, h, w)` tuple of a resident batch; bgr=True when its bytes are
    B,G,R) -> the reference's phash strings, one per image."""
    return to_hex(engine.phash(images, bgr=bgr))


def phash_mixed(engine, images, order='rgb'):
    """Images that each have their own size (a list of uint8 [h,w,3] arrays, or `(device_pointers, sizes)` for resident images; order:
    'rgb' or 'bgr' bytes) -> uint64 [n], the hash `fe_phash` gives each image alone, from one `fe_phash_mixed` call. `to_hex` turns them
    into the reference's strings."""
    return engine.phash_mixed(images, order=order)
