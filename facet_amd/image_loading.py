"""Image loading: the reference's utils/image_loading.py `load_image_from_path` (:44-112) with the JPEG decode on the GPU.

    decode_jpegs(engine, blobs)            -> [uint8 [h,w,3] | None]   RGB pixels of each file, in input order
    load_image_from_path(engine, path)     -> (pil_img, img_cv)        the reference's signature, for one file
    decode_groups(engine, blobs, device)   -> the resident batches BatchScorer.process_files scores, and what is left for Pillow
Each takes progressive=False; True sends complete progressive files through the GPU decoder as well. Each takes parallel_entropy=False;
True decodes a baseline file's long entropy-coded segments with one GPU lane per 128 bytes instead of one per segment (Engine.jpeg_decode).

The reference opens every file with `Image.open`, `ImageOps.exif_transpose` and `convert('RGB')` (:100-103). `fe_jpeg_decode` gives those
pixels for baseline Huffman JPEG files (YCbCr 4:4:4 / 4:2:2 / 4:2:0 or grayscale, one scan, any tables, with or without restart markers,
all eight EXIF orientations) from the files' bytes, and with progressive=True for progressive Huffman files whose scans are a complete
normal progression (what `Image.save(progressive=True)`, jpegtran and the usual exporters write; libjpeg smooths anything less, which
stays with Pillow). Every other input - CMYK files, corrupt streams, PNG, anything the probe or the decode gives a non-zero status -
goes through that same Pillow recipe here, so the functions always return what the reference would, whatever `progressive` is, and
None where it returns (None, None). RAW files (CR2 / CR3) stay with the caller: rawpy is its dependency. progressive is off by default:
no rate of either entropy stage has been recorded on an MI355X yet (tools/perf_jpeg_decode.py measures both).
"""
import io
import os

import numpy as np

RAW_SUFFIXES = ('.cr2', '.cr3')

# status codes of Engine.jpeg_probe / jpeg_decode (FE_JPEG_* in include/facet_engine.h). With progressive=True a progressive file is
# 'ok' when its scans are a complete normal progression and 'other' (or a negative code) when they are not.
JPEG_STATUS = {0: 'ok', 1: 'progressive', 2: 'arithmetic', 3: 'precision', 4: 'components', 5: 'adobe_rgb', 6: 'sampling', 7: 'multiscan',
               8: 'other', -1: 'bad_marker', -2: 'bad_huffman', -3: 'premature_end', -4: 'bad_restart', -5: 'bad_dimensions',
               -6: 'bad_coefficient'}


def read_blob(path_or_blob):
    """bytes stay bytes; a path is read. CR2 / CR3 paths raise ValueError: RAW development stays with the caller."""
    if isinstance(path_or_blob, (bytes, bytearray, memoryview)):
        return bytes(path_or_blob)
    p = os.fspath(path_or_blob)
    if p.lower().endswith(RAW_SUFFIXES):
        raise ValueError(f"{p}: RAW files are not decoded here (the reference uses rawpy); pass the developed image instead")
    with open(p, 'rb') as f:
        return f.read()


def pillow_image(blob, scale=1):
    """utils/image_loading.py:100-103 on the file's bytes -> PIL RGB image, or None where the reference gives up. scale 2, 4, 8: a JPEG
    file is drafted to that scale first (what JpegImageFile.draft() sets when it chooses it); other formats have no draft mode."""
    from PIL import Image, ImageOps
    try:
        im = Image.open(io.BytesIO(blob))
        if scale != 1 and im.format == 'JPEG' and len(im.tile) == 1 and not im.decoderconfig:
            w, h = im.size
            im._size = (-(-w // scale), -(-h // scale))
            im.tile = [im.tile[0]._replace(extents=(0, 0) + im.size)]
            im.decoderconfig = (scale, 0)
        im = ImageOps.exif_transpose(im)
        if im.mode != 'RGB':
            im = im.convert('RGB')
        im.load()
        return im
    except Exception as e:
        print(f"Error loading image: {e}")
        return None


def pillow_rgb(blob, scale=1):
    im = pillow_image(blob, scale)
    return None if im is None else np.asarray(im, dtype=np.uint8)


def decode_groups(engine, blobs, device=False, progressive=False, scale=1, parallel_entropy=False):
    """Probe every file, group the decodable ones by output size and decode each group with one fe_jpeg_decode. progressive: a file the
    probe calls progressive (status 1) is probed again for the progressive decoder and, when that takes it, joins the group of its size.
    -> (groups, rest): groups = [(indices, pixels)], pixels a uint8 [k,h,w,3] array or with device=True a (device_ptr, k, h, w) tuple the
    caller frees, holding exactly the images of `indices` in that order; rest = the indices left for Pillow. scale 2, 4, 8: the decode
    at 1/scale (Engine.jpeg_decode's scale), grouped by scaled size. parallel_entropy: Engine.jpeg_decode's; the pixels do not depend on it."""
    if scale not in (1, 2, 4, 8):
        raise ValueError(f"decode_groups: scale {scale!r} (1, 2, 4 or 8)")
    sizes, rest = {}, []
    for i, b in enumerate(blobs):
        info = engine.jpeg_probe(b)
        if progressive and info['status'] == 1:
            info = engine.jpeg_probe(b, progressive=True)
        if info['status'] != 0:
            rest.append(i)
            continue
        h, w = -(-info['height'] // scale), -(-info['width'] // scale)
        if info['orientation'] >= 5:
            h, w = w, h
        sizes.setdefault((h, w), []).append(i)
    groups = []
    flag = dict(progressive=True) if progressive else {}
    if scale != 1:
        flag['scale'] = scale
    if parallel_entropy:
        flag['parallel_entropy'] = True
    for (h, w), idx in sizes.items():
        px, status = engine.jpeg_decode([blobs[i] for i in idx], h, w, device=device, **flag)
        good = [k for k in range(len(idx)) if status[k] == 0]
        if len(good) < len(idx):      # rare: a stream that only the entropy decoder finds corrupt. The batch must have no holes.
            rest.extend(idx[k] for k in range(len(idx)) if status[k] != 0)
            if device:
                engine.dev_free(px[0])
                px = None
                if good:
                    px, status = engine.jpeg_decode([blobs[idx[k]] for k in good], h, w, device=True, **flag)
                    assert not status.any()
            else:
                px = px[good]
            idx = [idx[k] for k in good]
        if idx:
            groups.append((idx, px))
    return groups, sorted(rest)


def decode_jpegs(engine, blobs, progressive=False, scale=1, parallel_entropy=False):
    """The RGB pixels of every file (bytes), as uint8 [h,w,3] arrays in input order: what load_image_from_path's pil_img holds, None
    where it fails. progressive: decode complete progressive files on the GPU too; the result is the same either way. scale 2, 4, 8:
    the pixels of the file drafted to 1/scale (libjpeg's scaled decode), from the GPU or from Pillow alike; grayscale comes back as RGB.
    parallel_entropy: the GPU decodes inside a file's entropy-coded segments in parallel; the result is the same either way."""
    blobs = [bytes(b) for b in blobs]
    out = [None] * len(blobs)
    groups, rest = decode_groups(engine, blobs, device=False, progressive=progressive, scale=scale, parallel_entropy=parallel_entropy)
    for idx, px in groups:
        for k, i in enumerate(idx):
            out[i] = px[k]
    for i in rest:
        out[i] = pillow_rgb(blobs[i], scale)
    return out


def load_image_from_path(engine, photo_path, progressive=False, parallel_entropy=False):
    """(pil_img, img_cv): PIL RGB image and BGR array of one file, (None, None) on error - utils/image_loading.py:44-112 for non-RAW files."""
    from PIL import Image
    try:
        blob = read_blob(photo_path)
    except ValueError:
        raise
    except Exception as e:
        print(f"Error loading image {photo_path}: {e}")
        return None, None
    rgb = decode_jpegs(engine, [blob], progressive=progressive, parallel_entropy=parallel_entropy)[0]
    if rgb is None:
        return None, None
    return Image.fromarray(rgb), np.ascontiguousarray(rgb[..., ::-1])
