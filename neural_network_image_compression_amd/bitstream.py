"""Bitstream container and directory drivers around the device codec.

The reference's on-disk bitstream is a PNG: the 96-channel u8 latent is reinterpreted
(raw C-order reshape per plane) as a 3-channel ``(n, 4h, 8w, 3)`` image
(``ProClass._feed_batch``, utils.py:30-44) and saved by Pillow with ``optimize=True``
(``save_img``, utils.py:85-87).  ``compress``/``uncompress`` walk a directory with
``read_dataset`` (utils.py:89-120) in batches of 4 (utils.py:46-62).

The pack/unpack reshape runs on the GPU (``nic_pack_latent``/``nic_unpack_latent``); PNG
coding (zlib) stays on the host, outside the measured encode/decode surface.

Beside it stands the native ``.nic`` container (``container="nic"``): a static per-channel rANS
code of the latent, written and read on the device (``nic_rans_encode``/``nic_rans_decode``;
format in DESIGN.md), so the host only moves and writes finished files.  PNG stays the default
and the parity format.

Reconstructions are written by Pillow's encoder by default (``png_writer="pillow"``); with
``png_writer="device"`` the decoder side writes them with the device PNG writer
(``nic_png_device_encode``; format in DESIGN.md): the same pixels, files of its own bytes, and
the host again only moves and writes finished files.
"""
from __future__ import annotations

import io
import os
import re
from typing import List, Sequence, Tuple

import numpy as np

IMAGE_EXTS = ("png", "jpg", "jpeg", "gif", "pgm", "ppm", "bmp", "jp2")  # utils.py:94


def read_dataset(dataset_path: str) -> Tuple[List[np.ndarray], List[str]]:
    """utils.py:89-120: sorted directory listing, colour (3-D) images only, u8 arrays.

    Returns a list (images may differ in size; the reference's object-array path breaks
    under NumPy 2) and the file stems."""
    from PIL import Image

    imgs, names = [], []
    for fn in sorted(os.listdir(dataset_path)):
        if fn.split(".")[-1] in IMAGE_EXTS:
            with Image.open(os.path.join(dataset_path, fn)) as im:
                a = np.array(im)
            if a.ndim == 3:
                imgs.append(a.astype(np.uint8))
                names.append(".".join(fn.split(".")[:-1]))
    return imgs, names


def png_bytes(img: np.ndarray, optimize: bool = True) -> bytes:
    """Pillow PNG encoding as save_img (utils.py:87)."""
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG", optimize=optimize)
    return buf.getvalue()


PNG_MODES = {"pillow": 0, "tf": 1}  # nic.h NIC_PNG_PILLOW / NIC_PNG_TF


def _png_shape(images: np.ndarray, fn: str):
    a = np.ascontiguousarray(images, dtype=np.uint8)
    if a.ndim not in (3, 4) or (a.ndim == 4 and a.shape[3] != 3):
        raise ValueError(f"{fn}: expected (M, H, W) or (M, H, W, 3) images, got shape {a.shape}")
    return a, a.shape[0], a.shape[1], a.shape[2], 3 if a.ndim == 4 else 1


def png_sizes(images: np.ndarray, threads: int = 16, mode: str = "pillow") -> np.ndarray:
    """PNG byte counts of every u8 image of images (M, H, W) or (M, H, W, 3), computed natively
    on host threads (nic_png_encode without output).  mode "pillow": len(png_bytes(a)) byte for
    byte (save_img, utils.py:85-87); mode "tf": tf.image.encode_png(compression=-1)'s settings,
    what get_bpp sizes (training.py:12-21; parity with TF itself unpinned, nic.h)."""
    import ctypes

    from . import _lib

    a, m, h, w, ch = _png_shape(images, "png_sizes")
    out = np.empty(m, np.int64)
    if m:
        _lib.check(_lib.lib().nic_png_encode(a.ctypes.data_as(ctypes.c_void_p), m, h, w, ch, PNG_MODES[mode], None, 0,
                                             out.ctypes.data_as(ctypes.c_void_p), int(threads)), "nic_png_encode")
    return out


def png_encode(images: np.ndarray, threads: int = 16, mode: str = "pillow") -> List[bytes]:
    """The PNG files of every u8 image of images (M, H, W) or (M, H, W, 3), encoded natively on
    host threads (nic_png_encode); mode "pillow" is byte for byte Pillow's optimize=True file."""
    import ctypes

    from . import _lib

    a, m, h, w, ch = _png_shape(images, "png_encode")
    if m == 0:
        return []
    L = _lib.lib()
    stride = ctypes.c_int64()
    _lib.check(L.nic_png_bound(h, w, ch, PNG_MODES[mode], ctypes.byref(stride)), "nic_png_bound")
    buf = np.empty((m, stride.value), np.uint8)
    sizes = np.empty(m, np.int64)
    _lib.check(L.nic_png_encode(a.ctypes.data_as(ctypes.c_void_p), m, h, w, ch, PNG_MODES[mode],
                                buf.ctypes.data_as(ctypes.c_void_p), stride.value,
                                sizes.ctypes.data_as(ctypes.c_void_p), int(threads)), "nic_png_encode")
    return [buf[i, :sizes[i]].tobytes() for i in range(m)]


def save_img(img: np.ndarray, output_dir: str, filename: str) -> str:
    """utils.py:85-87 (the file Pillow's optimize=True writes, encoded natively)."""
    return save_imgs(np.asarray(img)[None], output_dir, [filename], threads=1)[0]


def save_imgs(imgs: np.ndarray, output_dir: str, filenames: Sequence[str], threads: int = 16) -> List[str]:
    """save_img (utils.py:85-87) of a batch of equal-shaped images: the PNG files encoded on
    ``threads`` native host threads (nic_png_encode, byte-identical to Pillow), then written."""
    imgs = np.asarray(imgs)
    assert (np.round(imgs) - imgs).sum() == 0  # utils.py:86
    return _write_files(png_encode(imgs.astype(np.uint8), threads=threads), output_dir, filenames, ".png")


def _write_files(datas: Sequence[bytes], output_dir: str, filenames: Sequence[str], ext: str) -> List[str]:
    paths = []
    for data, name in zip(datas, filenames):
        path = os.path.join(output_dir, name + ext)
        with open(path, "wb") as f:
            f.write(data)
        paths.append(path)
    return paths


def png_bpp(packed: np.ndarray, pixels: int, optimize: bool = True) -> float:
    """training.py:12-21 / training.py:157-163: 8 * len(PNG) / pixels of the original image."""
    return 8.0 * len(png_bytes(packed, optimize)) / float(pixels)


CONTAINERS = ("png", "nic")
NIC_SEG_PIXELS = 32  # latent pixels per rANS segment (one device lane each) of the files written here


def _inspect(ver: int, data: bytes) -> tuple:
    """nic_rans_inspect (ver 1: three ints) or nic_rans2_inspect / nic_rans3_inspect (five ints and
    the prior id) on data: the values, or ValueError with the call's text."""
    import ctypes

    from . import _lib

    a = np.frombuffer(data, np.uint8)
    v = [ctypes.c_int() for _ in range(3 if ver == 1 else 5)]
    pid = ctypes.c_uint32()
    fn = getattr(_lib.lib(), {1: "nic_rans_inspect", 2: "nic_rans2_inspect", 3: "nic_rans3_inspect"}[ver])
    rc = fn(a.ctypes.data_as(ctypes.c_void_p), len(data), *[ctypes.byref(t) for t in v],
            *([] if ver == 1 else [ctypes.byref(pid)]))
    if rc != _lib.NIC_OK:
        raise ValueError(f"[{rc}] {_lib.last_error()}")
    return tuple(t.value for t in v) + (() if ver == 1 else (int(pid.value),))


def nic_inspect(data: bytes) -> Tuple[int, int, int]:
    """(h8, w8, seg_pixels) of a well-formed .nic file; ValueError (nic_rans_inspect's text)
    otherwise.  Host only."""
    return _inspect(1, data)


def nic2_inspect(data: bytes) -> Tuple[int, int, int, int, int, int]:
    """(h8, w8, seg_pixels, H, W, prior_id) of a well-formed version-2 .nic file; ValueError
    (nic_rans2_inspect's text) otherwise.  Host only."""
    return _inspect(2, data)


def nic3_inspect(data: bytes) -> Tuple[int, int, int, int, int, int]:
    """(h8, w8, seg_pixels, H, W, prior_id) of a well-formed version-3 .nic file; ValueError
    (nic_rans3_inspect's text) otherwise.  Host only."""
    return _inspect(3, data)


def _download_files(buf, sizes) -> List[bytes]:
    """Files buf[i, :sizes[i]] of an (N, stride) u8 device tensor as bytes, in one copy to the host."""
    if buf.shape[0] == 0:
        return []
    sizes = sizes.cpu().numpy()
    host = buf[:, :int(sizes.max())].contiguous().cpu().numpy()
    return [host[i, :sizes[i]].tobytes() for i in range(host.shape[0])]


def nic_files(codec, z, seg_pixels: int = NIC_SEG_PIXELS, size=None) -> List[bytes]:
    """The .nic file of every latent of z (N,h,w,96), a u8 tensor on the codec's device: coded
    and assembled there (Codec.rans_encode), then one copy of the files to the host.  With a
    context prior set on the codec the files are version 3 (Codec.rans3_encode); else with a
    prior set they are version 2 (Codec.rans2_encode); both record the images' size=(H, W)
    (default 8h x 8w).  Without either they are version 1 and size is not stored."""
    if codec.context_prior is not None:
        buf, sizes = codec.rans3_encode(z, seg_pixels, size)
    elif codec.prior is not None:
        buf, sizes = codec.rans2_encode(z, seg_pixels, size)
    else:
        buf, sizes = codec.rans_encode(z, seg_pixels)
    return _download_files(buf, sizes)


def _inspect_any(codec, i: int, data: bytes, who: str = "read_nic"):
    """The decode group and the image size of file i: byte 4 says which version's checks apply.
    A version-2 file also needs the codec's prior to be the one it was written under, a version-3
    file the codec's context prior.  who: the caller named in the ValueError."""
    try:
        if len(data) > 4 and data[4] in (2, 3):
            ver = data[4]
            h8, w8, _, H, W, pid = (nic2_inspect if ver == 2 else nic3_inspect)(data)
            have = codec.prior if ver == 2 else codec.context_prior
            if have is None or have.id != pid:
                raise ValueError(f"written under prior {pid:08x}, the codec's prior is "
                                 + ("not set" if have is None else f"{have.id:08x}"))
            return (ver, h8, w8), (H, W)
        h8, w8, sp = nic_inspect(data)
        return (1, h8, w8, sp), (8 * h8, 8 * w8)
    except ValueError as e:
        raise ValueError(f"{who}: file {i}: {e}") from None


def read_nic_sizes(codec, files: Sequence[bytes]) -> List[Tuple[int, int]]:
    """The image size (H, W) each .nic file stands for: a version-2 or version-3 file's own,
    8 h8 x 8 w8 for a version-1 file (which does not record it).  The same host checks as read_nic."""
    return [_inspect_any(codec, i, data)[1] for i, data in enumerate(files)]


def read_nic(codec, files: Sequence[bytes], sizes: bool = False) -> list:
    """The latents of .nic files: a list of (h8,w8,96) u8 tensors on the codec's device, in the
    files' order.  Every file is checked on the host first (nic_inspect, or nic2_inspect /
    nic3_inspect for a version-2 / version-3 file: ValueError naming the file's index); version-1
    files of equal (h8, w8, seg_pixels) and version-2 or version-3 files of equal (h8, w8) are
    decoded as one device batch each.
    sizes=True: also the files' image sizes, (latents, [(H, W)])."""
    groups, hw = {}, []
    for i, data in enumerate(files):
        key, size = _inspect_any(codec, i, data)
        groups.setdefault(key, []).append(i)
        hw.append(size)
    out = [None] * len(files)
    for key, idx in groups.items():
        buf, lens = _upload_files(codec, [files[i] for i in idx])
        try:
            decode = {1: codec.rans_decode, 2: codec.rans2_decode, 3: codec.rans3_decode}[key[0]]
            z = decode(buf, lens, key[1], key[2])
        except ValueError as e:
            raise ValueError(f"read_nic: files {idx}: {e}") from None
        for r, i in enumerate(idx):
            out[i] = z[r]
    return (out, hw) if sizes else out


def _upload_files(codec, files: Sequence[bytes]):
    """The files as one zero-padded (N, stride) u8 device tensor and their (N,) int64 sizes."""
    import torch

    stride = max(len(d) for d in files)
    host = np.zeros((len(files), stride), np.uint8)
    for r, d in enumerate(files):
        host[r, :len(d)] = np.frombuffer(d, np.uint8)
    lens = torch.tensor([len(d) for d in files], dtype=torch.int64)
    dev = f"cuda:{codec.device}"
    return torch.from_numpy(host).to(dev), lens.to(dev)


def _group_text(key) -> str:
    return f"version {key[0]}, latent {key[1]}x{key[2]}" + (f", seg_pixels {key[3]}" if key[0] == 1 else "")


def read_nic_window(codec, files: Sequence[bytes], window, sizes: bool = False):
    """The window = (r0, c0, rows, cols) of the latents of .nic files: one (N,rows,cols,96) u8 tensor
    on the codec's device, read_nic's latents cut to [r0:r0+rows, c0:c0+cols] -- but only the segments
    that hold a pixel of the window are entropy-decoded (Codec.rans*_decode_window).  The host checks
    are read_nic's (ValueError naming the file's index).  The files are one device batch: they must
    share the version and (h8, w8), version-1 files also seg_pixels, as read_nic groups them
    (ValueError naming the first file that differs from file 0).  Whole files are uploaded.
    sizes=True: also the files' image sizes, (window latents, [(H, W)])."""
    import torch

    r0, c0, rows, cols = (int(v) for v in window)
    keys, hw = [], []
    for i, data in enumerate(files):
        key, size = _inspect_any(codec, i, data, "read_nic_window")
        if keys and key != keys[0]:
            raise ValueError(f"read_nic_window: file {i}: {_group_text(key)}, but file 0 is {_group_text(keys[0])}: "
                             "the files of one call must decode as one batch")
        keys.append(key)
        hw.append(size)
    if not files:
        z = torch.empty((0, max(rows, 0), max(cols, 0), 96), dtype=torch.uint8, device=f"cuda:{codec.device}")
        return (z, hw) if sizes else z
    ver, h8, w8 = keys[0][:3]
    buf, lens = _upload_files(codec, files)
    try:
        decode = {1: codec.rans_decode_window, 2: codec.rans2_decode_window, 3: codec.rans3_decode_window}[ver]
        z = decode(buf, lens, h8, w8, (r0, c0, rows, cols))
    except ValueError as e:
        raise ValueError(f"read_nic_window: {e}") from None
    return (z, hw) if sizes else z


def _fits(box, size) -> bool:
    y, x, h, w = box
    return y >= 0 and x >= 0 and h >= 1 and w >= 1 and y + h <= size[0] and x + w <= size[1]


def _files_and_names(files: Sequence):
    """The bytes of files given as bytes or as paths to read, and what an error calls each: its path, or "file i"."""
    datas, names = [], []
    for i, f in enumerate(files):
        is_path = isinstance(f, (str, os.PathLike))
        datas.append(_read_bytes(os.fspath(f)) if is_path else bytes(f))
        names.append(os.fspath(f) if is_path else f"file {i}")
    return datas, names


def _region_of_batch(decoder, files: Sequence[bytes], size, box):
    """decode_region's device part for files that decode as one batch and whose images hold the box."""
    codec = decoder.codec
    window, (oy, ox) = codec.region_plan(size[0], size[1], box)
    rec = codec.decode(read_nic_window(codec, files, window))
    return rec[:, oy:oy + box[2], ox:ox + box[3]].contiguous()


def decode_region(decoder, files: Sequence, box):
    """The pixel box = (y, x, h, w) of the images of .nic files (bytes, or paths to read): an (N,h,w,3)
    u8 tensor on the decoder's device, equal to the box cut out of the whole reconstructions.  The box
    is checked against every file's recorded H x W (8 h8 x 8 w8 for a version-1 file; ValueError
    naming the file when it does not fit), Codec.region_plan gives the latent window that holds every
    latent pixel the box depends on (NIC_DECODE_HALO), read_nic_window entropy-decodes only that
    window's segments, the decoder runs on the window, and the box is cut on the device.  The files
    must decode as one batch (read_nic_window)."""
    import torch

    box = tuple(int(v) for v in box)
    if len(box) != 4:
        raise ValueError(f"decode_region: box must be (y, x, h, w), got {box!r}")
    datas, names = _files_and_names(files)
    hw = []
    for i, data in enumerate(datas):
        try:
            size = _inspect_any(decoder.codec, i, data, "decode_region")[1]
        except ValueError as e:
            raise ValueError(f"{names[i]}: {e}") from None
        if not _fits(box, size):
            raise ValueError(f"decode_region: {names[i]}: box (y {box[0]}, x {box[1]}, {box[2]} x {box[3]}) does not lie "
                             f"inside its {size[0]} x {size[1]} image")
        hw.append(size)
    if not datas:
        return torch.empty((0, max(box[2], 0), max(box[3], 0), 3), dtype=torch.uint8, device=f"cuda:{decoder.codec.device}")
    return _region_of_batch(decoder, datas, hw[0], box)


def _window_groups(codec, files: Sequence[bytes], boxes, who: str, names: Sequence[str]):
    """The host part of read_nic_windows and decode_regions: every check, then the plans.  Returns the
    boxes' (h, w) and the groups as {(rows, cols): [(file index, (h8, w8, r0, c0), (off_y, off_x))]},
    in the order the window shapes first appear."""
    boxes = [tuple(int(v) for v in b) for b in boxes]
    if len(boxes) != len(files):
        raise ValueError(f"{who}: {len(boxes)} boxes for {len(files)} files: one box (y, x, h, w) per file")
    for i, b in enumerate(boxes):
        if len(b) != 4:
            raise ValueError(f"{who}: {names[i]}: box must be (y, x, h, w), got {b!r}")
        if b[2:] != boxes[0][2:]:
            raise ValueError(f"{who}: {names[i]}: box size {b[2]} x {b[3]}, but the first box is {boxes[0][2]} x "
                             f"{boxes[0][3]}: the boxes of one call must share one size")
    groups, ver0 = {}, None
    for i, data in enumerate(files):
        try:
            key, size = _inspect_any(codec, i, data, who)
        except ValueError as e:
            raise ValueError(f"{names[i]}: {e}") from None
        if ver0 is None:
            ver0 = key[0]
        if key[0] != ver0:
            raise ValueError(f"{who}: {names[i]}: version {key[0]}, but {names[0]} is version {ver0}: the files of one "
                             "call must share the container version")
        b = boxes[i]
        if not _fits(b, size):
            raise ValueError(f"{who}: {names[i]}: box (y {b[0]}, x {b[1]}, {b[2]} x {b[3]}) does not lie inside its "
                             f"{size[0]} x {size[1]} image")
        win, off = codec.region_plan_fixed(size[0], size[1], b)
        groups.setdefault(win[2:], []).append((i, (key[1], key[2], win[0], win[1]), off))
    return (boxes[0][2:] if boxes else (0, 0)), ver0, groups


def _read_window_groups(codec, files: Sequence[bytes], ver: int, groups, who: str, names: Sequence[str]):
    """One upload and one Codec.rans*_decode_windows per group: [(file indices, (n,rows,cols,96) latents, offsets)]."""
    decode = {1: codec.rans_decode_windows, 2: codec.rans2_decode_windows, 3: codec.rans3_decode_windows}.get(ver)
    out = []
    for shape, members in groups.items():
        idx = [m[0] for m in members]
        buf, lens = _upload_files(codec, [files[i] for i in idx])
        try:
            z = decode(buf, lens, [m[1] for m in members], shape)
        except ValueError as e:  # the device refused a file of the group: "image k" counts inside the group
            m = re.search(r"image (\d+)", str(e))
            which = names[idx[int(m.group(1))]] if m and int(m.group(1)) < len(idx) else f"files {idx}"
            raise ValueError(f"{who}: {which}: {e}") from None
        out.append((idx, z, [m[2] for m in members]))
    return out


def read_nic_windows(codec, files: Sequence[bytes], boxes):
    """The latent windows that pixel boxes need, one box (y, x, h, w) per .nic file, all boxes of one
    (h, w); the files may hold images of different sizes.  Codec.region_plan_fixed gives every file a
    window whose shape depends on the box size alone -- unless the file's latent is smaller than that
    in a dimension, which gives it another shape -- so the files are grouped by window shape and each
    group is uploaded and entropy-decoded as one device batch (Codec.rans*_decode_windows: only the
    segments that hold a pixel of a file's window).  Returns one entry per group, in the order the
    shapes first appear: (the files' indices, their (n,rows,cols,96) u8 window latents on the codec's
    device, their [(off_y, off_x)]: where each box starts in its window's reconstruction).
    The host checks are read_nic's (ValueError naming the file's index); the files must share the
    container version, every box must lie inside its file's recorded H x W (8 h8 x 8 w8 for a
    version-1 file), and the boxes must share their size (ValueError naming the file).  Whole files
    are uploaded."""
    names = [f"file {i}" for i in range(len(files))]
    _, ver, groups = _window_groups(codec, files, boxes, "read_nic_windows", names)
    return _read_window_groups(codec, files, ver, groups, "read_nic_windows", names)


def decode_regions(decoder, files: Sequence, boxes):
    """One pixel box (y, x, h, w) per .nic file (bytes, or paths to read), all boxes of one (h, w), out
    of files whose images may differ in size: an (N,h,w,3) u8 tensor on the decoder's device, in the
    files' order, each the box cut out of that file's whole reconstruction.  read_nic_windows' checks
    and groups (ValueError naming the file, by its path where it was given as one); per group the
    window entropy decode, the decoder on the (n,rows,cols,96) windows and Codec.cut_boxes, all on the
    device.  Files no smaller than the fixed window -- every file, for a directory of images larger
    than the crop -- are one group, so one batch, whatever their sizes."""
    import torch

    datas, names = _files_and_names(files)
    codec = decoder.codec
    (h, w), ver, groups = _window_groups(codec, datas, boxes, "decode_regions", names)
    out = None
    for idx, z, offs in _read_window_groups(codec, datas, ver, groups, "decode_regions", names):
        cut = codec.cut_boxes(codec.decode(z), offs, h, w)
        if len(idx) == len(datas):  # one group: its order is the files'
            return cut
        if out is None:
            out = torch.empty((len(datas), h, w, 3), dtype=torch.uint8, device=cut.device)
        out[torch.tensor(idx, device=cut.device)] = cut
    if out is None:
        out = torch.empty((0, max(h, 0), max(w, 0), 3), dtype=torch.uint8, device=f"cuda:{codec.device}")
    return out


def _window_groups_any(codec, files: Sequence[bytes], boxes, bucket, who: str, names: Sequence[str]):
    """_window_groups for boxes of any sizes: its checks without the equal-size one, then
    Codec.region_plan_window towards the call's one target shape (bucket None) or each box's own need
    rounded up to multiples of bucket.  Returns the boxes, the version and the groups, as there."""
    boxes = [tuple(int(v) for v in b) for b in boxes]
    if len(boxes) != len(files):
        raise ValueError(f"{who}: {len(boxes)} boxes for {len(files)} files: one box (y, x, h, w) per file")
    if bucket is not None and (isinstance(bucket, bool) or not isinstance(bucket, int) or bucket < 1):
        raise ValueError(f"{who}: bucket must be None or an int >= 1, got {bucket!r}")
    sizes, keys, ver0 = [], [], None
    for i, (data, b) in enumerate(zip(files, boxes)):
        if len(b) != 4:
            raise ValueError(f"{who}: {names[i]}: box must be (y, x, h, w), got {b!r}")
        try:
            key, size = _inspect_any(codec, i, data, who)
        except ValueError as e:
            raise ValueError(f"{names[i]}: {e}") from None
        if ver0 is None:
            ver0 = key[0]
        if key[0] != ver0:
            raise ValueError(f"{who}: {names[i]}: version {key[0]}, but {names[0]} is version {ver0}: the files of one "
                             "call must share the container version")
        if not _fits(b, size):
            raise ValueError(f"{who}: {names[i]}: box (y {b[0]}, x {b[1]}, {b[2]} x {b[3]}) does not lie inside its "
                             f"{size[0]} x {size[1]} image")
        sizes.append(size)
        keys.append(key)
    needs = [codec.window_need(b[2], b[3]) for b in boxes]
    if bucket is None:
        one = (max((r for r, _ in needs), default=0), max((c for _, c in needs), default=0))
        targets = [one] * len(needs)
    else:
        targets = [(-(-r // bucket) * bucket, -(-c // bucket) * bucket) for r, c in needs]
    groups = {}
    for i, (b, size, key, target) in enumerate(zip(boxes, sizes, keys, targets)):
        win, off = codec.region_plan_window(size[0], size[1], b, target)
        groups.setdefault(win[2:], []).append((i, (key[1], key[2], win[0], win[1]), off))
    return boxes, ver0, groups


def read_nic_windows_any(codec, files: Sequence[bytes], boxes, bucket=None):
    """read_nic_windows for boxes of different sizes: one box (y, x, h, w) per .nic file, the same
    checks without the equal-size one, the same result -- one (file indices, (n,rows,cols,96) window
    latents, [(off_y, off_x)]) per group of one window shape.  bucket None (the default): the call has
    one target shape, the largest rows and the largest columns any box needs (Codec.window_need), and
    Codec.region_plan_window plans every box towards it, so the files form one group unless a latent
    is smaller than the target in a dimension; a window larger than its box needs changes no pixel of
    the box.  bucket = q (an int >= 1): every box's own need is rounded up to multiples of q and the
    files are grouped by the result: smaller windows, more groups, each of which pays the entropy
    stage's fixed cost."""
    names = [f"file {i}" for i in range(len(files))]
    _, ver, groups = _window_groups_any(codec, files, boxes, bucket, "read_nic_windows_any", names)
    return _read_window_groups(codec, files, ver, groups, "read_nic_windows_any", names)


def decode_crops(decoder, files: Sequence, boxes, size, flip=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), dtype=None,
                 bucket=None):
    """One pixel box (y, x, h, w) per .nic file (bytes, or paths to read), the boxes of any sizes: every
    box is cut out of its file's reconstruction, resized to size = (oh, ow) as F.interpolate(mode=
    "bilinear", antialias=True) resizes float input, mirrored left to right where flip[i] is true,
    and returned as (N, 3, oh, ow) torch.float32 (the default) or torch.float16 holding (v / 255 -
    mean[c]) / std[c], or as (N, oh, ow, 3) torch.uint8, on the decoder's device, in the files' order.
    read_nic_windows_any's checks and groups (ValueError naming the file, by its path where it was
    given as one; bucket as there); per group one upload, one window entropy decode, the decoder on
    the (n,rows,cols,96) windows and one Codec.resample_boxes, which writes the group's images into
    their places of the one result."""
    import torch

    who = "decode_crops"
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.float16, torch.uint8):
        raise ValueError(f"{who}: dtype {dtype} is not torch.float32, torch.float16 or torch.uint8")
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: size must be (oh, ow), got {size!r}") from None
    if not (1 <= oh <= 16384 and 1 <= ow <= 16384):
        raise ValueError(f"{who}: size {oh} x {ow} not in 1..16384")
    mean64, std64 = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    if mean64.shape != (3,) or std64.shape != (3,) or not np.all(np.isfinite(mean64)) or not np.all(np.isfinite(std64)) \
            or np.any(std64 == 0):
        raise ValueError(f"{who}: mean and std must be 3 finite numbers each, std not 0; got {mean!r}, {std!r}")
    datas, names = _files_and_names(files)
    flips = [0] * len(datas) if flip is None else [int(bool(f)) for f in flip]
    if len(flips) != len(datas):
        raise ValueError(f"{who}: {len(flips)} flips for {len(datas)} files: one per file, or None")
    codec = decoder.codec
    boxes, ver, groups = _window_groups_any(codec, datas, boxes, bucket, who, names)
    shape = (len(datas), oh, ow, 3) if dtype == torch.uint8 else (len(datas), 3, oh, ow)
    out = torch.empty(shape, dtype=dtype, device=f"cuda:{codec.device}")
    for idx, z, offs in _read_window_groups(codec, datas, ver, groups, who, names):
        table = [(off[0], off[1], boxes[i][2], boxes[i][3], flips[i], i) for i, off in zip(idx, offs)]
        codec.resample_boxes(codec.decode(z), table, (oh, ow), dtype, mean, std, out=out)
    return out


PNG_WRITERS = ("pillow", "device")


def _check_png_writer(png_writer: str, decoder_side: bool) -> None:
    if png_writer not in PNG_WRITERS:
        raise ValueError(f"png_writer must be one of {PNG_WRITERS}, got {png_writer!r}")
    if png_writer == "device" and not decoder_side:
        raise ValueError('png_writer="device" applies to the decoder side only: the compressed PNG is the reference '
                         "bitstream and stays Pillow's bytes")


def png_files_device(codec, x, filter="adaptive") -> List[bytes]:
    """The PNG file of every image of x (N,H,W,3) or (N,H,W,1), a u8 tensor on the codec's device:
    filtered, coded and framed there (Codec.png_encode), then one copy of the files to the host."""
    return _download_files(*codec.png_encode(x, filter))


PNG_READERS = ("pillow", "device")
_PNG_SIGNATURE = bytes([137, 80, 78, 71, 13, 10, 26, 10])


def _check_png_reader(png_reader: str, container: str, decoder_side: bool) -> None:
    if png_reader not in PNG_READERS:
        raise ValueError(f"png_reader must be one of {PNG_READERS}, got {png_reader!r}")
    if png_reader == "device" and container == "nic" and decoder_side:
        raise ValueError('png_reader="device" does not apply to the decoder side of container="nic": it reads .nic '
                         "files, no PNG")


class PngUnsupported(ValueError):
    """nic_png_inspect: a well-formed PNG of a kind the device reader does not take (NIC_EUNSUPPORTED)."""


def png_stream(data: bytes) -> Tuple[int, int, int, bytes]:
    """(h, w, channels, zlib stream) of one PNG file's bytes: nic_png_inspect checks the signature, the
    chunk framing and every CRC-32 on the host and cuts out the concatenated IDAT payload, which is
    what Codec.png_read takes.  ValueError for a broken file (NIC_ECORRUPT), PngUnsupported for a
    well-formed one the device reader does not take (interlaced, 16-bit, palette, alpha, tRNS, rows
    over 16,384 bytes); both carry the call's text.  Host only."""
    import ctypes

    from . import _lib

    a = np.frombuffer(data, np.uint8)
    h, w, ch, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    out = np.empty(max(len(data), 1), np.uint8)
    rc = _lib.lib().nic_png_inspect(a.ctypes.data_as(ctypes.c_void_p), len(data), ctypes.byref(h), ctypes.byref(w),
                                    ctypes.byref(ch), out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n))
    if rc == _lib.NIC_EUNSUPPORTED:
        raise PngUnsupported(f"[{rc}] {_lib.last_error()}")
    if rc != _lib.NIC_OK:
        raise ValueError(f"[{rc}] {_lib.last_error()}")
    return h.value, w.value, ch.value, out[:n.value].tobytes()


class _PngStream:
    """One PNG file for the device reader; shape / ndim are those of the array Pillow would give."""

    def __init__(self, h: int, w: int, channels: int, data: bytes):
        self.hwc, self.data = (h, w, channels), data
        self.shape = (h, w, channels) if channels != 1 else (h, w)
        self.ndim = len(self.shape)


def _png_item(data: bytes, name: str):
    """A file's bytes -> a _PngStream when it is a PNG the device reader takes, else Pillow's array
    (JPEGs and the other formats; unsupported PNGs).  ValueError naming the file for a corrupt PNG."""
    from PIL import Image

    if data[:8] == _PNG_SIGNATURE:
        try:
            return _PngStream(*png_stream(data))
        except PngUnsupported:
            pass
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im)


def _read_item(path: str):
    return _png_item(_read_bytes(path), path)


def _stage_batch(codec, items: Sequence, names: Sequence[str]):
    """Equal-shaped items (_PngStream or Pillow's arrays) -> one (N,h,w,c) u8 tensor on the codec's
    device: the streams staged in one pinned buffer, copied in one transfer and read by
    Codec.png_read; the arrays stacked and uploaded.  ValueError naming the file the device refuses."""
    import torch

    dev = f"cuda:{codec.device}"
    zi = [k for k, it in enumerate(items) if isinstance(it, _PngStream)]
    ai = [k for k, it in enumerate(items) if not isinstance(it, _PngStream)]
    imgs = arr = None
    if zi:
        h, w, ch = items[zi[0]].hwc
        stride = max(1, max(len(items[k].data) for k in zi))
        host = torch.zeros((len(zi), stride), dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        for r, k in enumerate(zi):
            view[r, :len(items[k].data)] = np.frombuffer(items[k].data, np.uint8)
        lens = torch.tensor([len(items[k].data) for k in zi], dtype=torch.int64)
        try:
            imgs, _ = codec.png_read(host.to(dev, non_blocking=True), lens.to(dev), h, w, ch)
        except ValueError as e:
            m = re.search(r"image (\d+)", str(e))
            which = names[zi[int(m.group(1))]] if m and int(m.group(1)) < len(zi) else f"files {list(names)}"
            raise ValueError(f"{which}: {e}") from None
        if not ai:
            return imgs
    if ai:
        a = np.stack([np.asarray(items[k], np.uint8) for k in ai])
        arr = torch.from_numpy(a.reshape(a.shape[0], a.shape[1], a.shape[2], -1)).to(dev)
        if not zi:
            return arr
    out = torch.empty((len(items),) + tuple(imgs.shape[1:]), dtype=torch.uint8, device=dev)
    out[torch.tensor(zi, device=dev)] = imgs
    out[torch.tensor(ai, device=dev)] = arr
    return out


def read_png_device(codec, files: Sequence[bytes]) -> list:
    """Image files' bytes -> their pixels on the codec's device, one tensor per shape group:
    [(the files' indices, (n,h,w,c) u8 tensor)], in the order the shapes first appear (gray: c = 1).
    PNG files go through png_stream and, group by group, through one pinned staging buffer, one
    transfer and Codec.png_read; a file the inspector calls unsupported (and any other format) is
    decoded by Pillow and joins the group of its shape.  ValueError naming the file ("file i") for a
    corrupt PNG, on the host or on the device."""
    groups = {}
    items = []
    for i, data in enumerate(files):
        it = _png_item(bytes(data), f"file {i}")
        items.append(it)
        shape = tuple(it.shape) if len(it.shape) == 3 else tuple(it.shape) + (1,)
        groups.setdefault(shape, []).append(i)
    return [(idx, _stage_batch(codec, [items[i] for i in idx], [f"file {i}" for i in idx])) for idx in groups.values()]


def _batches(shapes: Sequence[tuple], batch_size: int):
    """Consecutive runs of equal-shaped images, at most batch_size long (utils.py:53-62)."""
    i = 0
    while i < len(shapes):
        j = i + 1
        while j < len(shapes) and j - i < batch_size and shapes[j] == shapes[i]:
            j += 1
        yield i, j
        i = j


def feed_batch(model, x: np.ndarray, filenames: Sequence[str], output_dir: str, in_cshape: int,
               pool=None, png_threads: int = 16, container: str = "png", png_writer: str = "pillow", rdoq=None) -> list:
    """utils.py:30-44 for one batch: unpack (decoder side), run the codec, pack (encoder side), save.

    The batch's PNG files are encoded natively on ``png_threads`` host threads (nic_png_encode,
    byte-identical to Pillow's optimize=True).  With a pool the encode + write is submitted to
    it and its future returned, so the caller runs the next batch on the GPU meanwhile.

    container "nic" (encoder side): the latents are coded into .nic files on the device
    (nic_files), copied to the host once, and the writer only writes them.

    png_writer "device" (decoder side): the reconstructions are made into PNG files on the device
    (png_files_device) and never reach the host as pixels; the writer only writes them.

    rdoq (encoder side of container "nic", a prior set on the codec): the codes are chosen by
    distortion + rdoq x bits under that prior (Encoder.encode_rdoq) before nic_files codes them."""
    import torch

    codec = model.codec
    # a batch the device PNG reader made is on the device already
    dev = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{codec.device}")
    n, h, w, c = dev.shape
    if in_cshape == 96 and c == 3:
        dev = codec.unpack(dev)
    out = model._device_call(dev) if rdoq is None else model.encode_rdoq(dev, rdoq, NIC_SEG_PIXELS)
    if container == "nic" and out.shape[-1] == 96:
        datas = nic_files(codec, out, size=(h, w))  # versions 2 and 3 (a prior is set) record the images' own size
        if pool is None:
            _write_files(datas, output_dir, filenames, ".nic")
            return []
        return [pool.submit(_write_files, datas, output_dir, list(filenames), ".nic")]
    if png_writer == "device" and out.shape[-1] == 3:
        datas = png_files_device(codec, out)
        if pool is None:
            _write_files(datas, output_dir, filenames, ".png")
            return []
        return [pool.submit(_write_files, datas, output_dir, list(filenames), ".png")]
    if out.shape[-1] == 96:
        out = codec.pack(out)
    host = out.cpu().numpy()
    if host.shape[1] == 1 or host.shape[2] == 1:  # np.squeeze (utils.py:44) changes the mode
        for i in range(host.shape[0]):
            a = np.squeeze(host[i])
            save_imgs(a[None], output_dir, [filenames[i]], threads=1)
        return []
    imgs = host
    if pool is None:
        save_imgs(imgs, output_dir, filenames, threads=png_threads)
        return []
    return [pool.submit(save_imgs, imgs, output_dir, list(filenames), png_threads)]


def list_dataset(dataset_path: str) -> List[str]:
    """utils.py:92-94: the sorted directory entries with an image extension."""
    return [fn for fn in sorted(os.listdir(dataset_path)) if fn.split(".")[-1] in IMAGE_EXTS]


def _read_one(path: str):
    from PIL import Image

    with Image.open(path) as im:
        return np.array(im)


def _host_threads() -> int:
    try:
        return max(1, len(os.sched_getaffinity(0)))
    except AttributeError:  # pragma: no cover
        return max(1, os.cpu_count() or 1)


WRITES_IN_FLIGHT = 2  # batches handed to the PNG writer and not yet written (use_model)
BATCH_PIXELS = 64 * 512 * 768  # pixels staged per device batch (use_model): 64 Kodak-sized images, 3 4K frames


RESIZE_POOL_BYTES = 1 << 29  # source bytes staged per device batch of resize= (use_model): 64 photographs of 2.8 megapixels


def _check_resize(resize, resize_mode: str):
    from .codec import FIT_MODES

    try:
        oh, ow = (int(v) for v in resize)
    except (TypeError, ValueError):
        raise ValueError(f"resize must be (oh, ow), got {resize!r}") from None
    if not (1 <= oh <= 16384 and 1 <= ow <= 16384):
        raise ValueError(f"resize {oh} x {ow} not in 1..16384")
    if resize_mode not in FIT_MODES:
        raise ValueError(f"resize_mode must be one of {FIT_MODES}, got {resize_mode!r}")
    return oh, ow


def resize_batch(codec, images: Sequence[np.ndarray], names: Sequence[str], size, mode: str = "center"):
    """Host images of any sizes -> one (N, oh, ow, 3) u8 tensor on the codec's device: one pool, one
    upload, one Codec.resample_ragged from the boxes codec.fit_boxes(shapes, size, mode).  ValueError
    naming the file that is not an (H, W, 3) image."""
    import torch

    from .codec import fit_boxes

    for a, name in zip(images, names):
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"{name}: resize takes (H, W, 3) images, got shape {tuple(a.shape)}")
    boxes = fit_boxes([a.shape[:2] for a in images], size, mode)
    return codec.resample_ragged(list(images), boxes, size, dtype=torch.uint8)


def _set_any_prior(codec, prior) -> None:
    """prior= of the drivers: a prior.Prior or a .nicp path sets the codec's prior (version 2), a
    prior.ContextPrior or a .nicc path its context prior (version 3); a path by its magic."""
    from .prior import ContextPrior, as_any_prior

    prior = as_any_prior(prior)
    if isinstance(prior, ContextPrior):
        codec.set_context_prior(prior)
    else:
        codec.set_prior(prior)


def use_model(model, dataset_path: str, checkpoint_path: str, output_dir: str, in_cshape: int,
              batch_size: int = 64, workers=None, container: str = "png", png_writer: str = "pillow",
              prior=None, region=None, png_reader: str = "pillow", resize=None, resize_mode: str = "center",
              rdoq=None) -> None:
    """utils.py:46-62: every colour image of ``dataset_path`` (sorted; read_dataset's filter)
    through the codec into ``output_dir``, one PNG per image named after its source.

    ``workers=0`` is the reference's serial loop (read everything, then batches of
    ``batch_size`` -- the reference's 4 -- each run and saved inline).  Otherwise (default) a
    pipeline over the host cores: images are decoded by a reader pool in file order, consecutive
    equal-shaped images are fed to the device ``batch_size`` (64) at a time (at most
    ``BATCH_PIXELS`` pixels), and each batch's PNG files are encoded natively on ``workers``
    threads (default: every CPU this process may use, at most 16) while the next batches are
    read and run; at most ``WRITES_IN_FLIGHT`` batches wait for the writer, so host memory stays
    bounded however large the directory.  Every image's output depends on that
    image alone (the kernels are batch-invariant), so the files are byte-identical either way.

    ``container="nic"``: the encoder side writes ``<stem>.nic`` files coded on the device instead
    of packed PNGs; the decoder side reads the directory's ``.nic`` files (sorted) and writes the
    same reconstruction PNGs (use_model_nic_in).

    ``png_writer="device"`` (decoder side only; ValueError on the encoder side, whose PNG is the
    reference bitstream): the reconstructions are written by the device PNG writer instead of
    Pillow's encoder -- the same pixels in files of other bytes.

    ``prior`` (a prior.Prior or a ``.nicp`` path; ``container="nic"`` only, ValueError otherwise):
    set on the model's codec for this and later calls.  The encoder side then writes version-2
    files, which carry each image's true H x W; the decoder side reads directories that mix both
    versions and crops the reconstructions of version-2 files to H x W.  A prior.ContextPrior or
    a ``.nicc`` path does the same with version 3 (a context prior takes precedence on the encoder
    side when the codec has both).  Without it everything behaves and writes as before.

    ``region`` (a pixel box (y, x, h, w); the decoder side of ``container="nic"`` only, ValueError
    otherwise: a packed PNG has no index to read a part of): every file is decoded to that box only
    (use_model_nic_in).

    ``png_reader="device"`` (ValueError on the decoder side of ``container="nic"``, which reads no
    PNG): the reader pool reads the files' bytes and runs nic_png_inspect on them (framing and every
    CRC-32); the PNG files it takes go to the device as zlib streams and are inflated and unfiltered
    there (Codec.png_read), JPEGs and the PNG kinds it does not take go through Pillow as before.
    File order, batching and the files written are those of ``"pillow"``.

    ``resize=(oh, ow)`` (the encoder side only, with ``png_reader="pillow"``; ValueError otherwise):
    the reader pool's images, of any sizes, are batched by count alone (``batch_size``, and at most
    ``RESIZE_POOL_BYTES`` of source pixels), go up as one pool and are resized to oh x ow on the device
    from the boxes ``codec.fit_boxes(shapes, resize, resize_mode)`` (resize_batch); what is encoded and
    written is the resized image, and version-2 and version-3 ``.nic`` files record oh x ow as its size.
    A colour image that is not (H, W, 3), such as RGBA, is a ValueError naming the file.

    ``rdoq=lam`` (the encoder side of ``container="nic"`` with a prior -- ``prior=`` or one set on the
    codec before -- and lam in [0, 16]; ValueError otherwise): every batch's codes are chosen by
    distortion + lam x bits under the prior its files are coded with, the context prior first
    (Encoder.encode_rdoq).  Without it nothing changes, not even the launches."""
    if container not in CONTAINERS:
        raise ValueError(f"container must be one of {CONTAINERS}, got {container!r}")
    _check_png_writer(png_writer, decoder_side=in_cshape == 96)
    _check_png_reader(png_reader, container, decoder_side=in_cshape == 96)
    if region is not None and not (container == "nic" and in_cshape == 96):
        raise ValueError('region applies to the decoder side of container="nic" only: a packed PNG has no index, '
                         "so a part of it cannot be decoded on its own")
    if resize is not None:
        if in_cshape != 3 or png_reader != "pillow":
            raise ValueError('resize applies to the encoder side with png_reader="pillow" only: it resizes the images '
                             "the reader pool decoded")
        resize = _check_resize(resize, resize_mode)
    if prior is not None:
        if container != "nic":
            raise ValueError('prior applies to container="nic" only: the PNG container has no entropy model')
        _set_any_prior(model.codec, prior)
    if rdoq is not None:
        if container != "nic" or in_cshape != 3:
            raise ValueError('rdoq applies to the encoder side of container="nic" only: it prices the codes under '
                             "the prior the .nic files are coded with")
        if model.codec.prior is None and model.codec.context_prior is None:
            raise ValueError("rdoq needs a prior: pass prior=, or set one on the codec")
        rdoq = float(rdoq)
        if not 0.0 <= rdoq <= model.codec.RDOQ_LAM_MAX:
            raise ValueError(f"rdoq {rdoq} not in [0, {model.codec.RDOQ_LAM_MAX:g}]")
    if container == "nic" and in_cshape == 96:
        more = {"region": region} if region is not None else {}
        return use_model_nic_in(model, dataset_path, checkpoint_path, output_dir, batch_size=batch_size, workers=workers,
                                png_writer=png_writer, **more)
    extra = {"container": container} if container != "png" else {}
    if png_writer != "pillow":
        extra["png_writer"] = png_writer
    if rdoq is not None:
        extra["rdoq"] = rdoq
    os.makedirs(output_dir, exist_ok=True)
    model.load(checkpoint_path)
    device_reader = png_reader == "device"
    if workers is not None and workers <= 0:
        if device_reader:
            pairs = [(_read_item(os.path.join(dataset_path, fn)), ".".join(fn.split(".")[:-1])) for fn in list_dataset(dataset_path)]
            imgs, names = [a for a, _ in pairs if a.ndim == 3], [s for a, s in pairs if a.ndim == 3]
        else:
            imgs, names = read_dataset(dataset_path)
        for i, j in _batches([a.shape if resize is None else () for a in imgs], batch_size):
            if resize is not None:
                x = resize_batch(model.codec, imgs[i:j], names[i:j], resize, resize_mode)
            else:
                x = _stage_batch(model.codec, imgs[i:j], names[i:j]) if device_reader else np.stack(imgs[i:j])
            feed_batch(model, x, names[i:j], output_dir, in_cshape, **extra)
        return
    from concurrent.futures import ThreadPoolExecutor

    threads = _host_threads()
    png_threads = int(workers) if workers else min(16, threads)
    files = list_dataset(dataset_path)
    with ThreadPoolExecutor(max_workers=min(8, threads)) as readers, ThreadPoolExecutor(max_workers=1) as writer:
        futures, batch, names, depth = [], [], [], 4 * max(1, batch_size)
        read = _read_item if device_reader else _read_one
        pending = [readers.submit(read, os.path.join(dataset_path, fn)) for fn in files[:depth]]

        def flush():
            if batch:
                # bounded host memory: at most WRITES_IN_FLIGHT batches' outputs wait for the
                # (slower) PNG writer; the device pass of the next batch still overlaps them
                while len(futures) >= WRITES_IN_FLIGHT:
                    futures.pop(0).result()  # re-raises a write error
                if resize is not None:
                    x = resize_batch(model.codec, batch, names, resize, resize_mode)
                else:
                    x = _stage_batch(model.codec, batch, names) if device_reader else np.stack(batch)
                futures.extend(feed_batch(model, x, list(names), output_dir, in_cshape, pool=writer,
                                          png_threads=png_threads, **extra))
                batch.clear()
                names.clear()
            while futures and futures[0].done():
                futures.pop(0).result()  # re-raise a write error early

        for k, fn in enumerate(files):
            a = pending[k].result()
            if k + depth < len(files):  # keep `depth` decodes in flight ahead of the device
                pending.append(readers.submit(read, os.path.join(dataset_path, files[k + depth])))
            pending[k] = None
            if a.ndim != 3:  # read_dataset keeps colour (3-D) images only
                continue
            if resize is not None:
                if batch and (len(batch) >= batch_size or sum(b.size for b in batch) + a.size > RESIZE_POOL_BYTES):
                    flush()
            elif batch and (a.shape != batch[0].shape or len(batch) >= batch_size
                            or (len(batch) + 1) * a.shape[0] * a.shape[1] > BATCH_PIXELS):
                flush()
            batch.append(a if isinstance(a, _PngStream) else a.astype(np.uint8, copy=False))
            names.append(".".join(fn.split(".")[:-1]))
        flush()
        for f in futures:
            f.result()  # re-raise any write error


def _read_bytes(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def use_model_nic_in(model, dataset_path: str, checkpoint_path: str, output_dir: str, batch_size: int = 64,
                     workers=None, png_writer: str = "pillow", prior=None, region=None) -> None:
    """The decoder side of ``container="nic"``: every ``.nic`` file of ``dataset_path`` (sorted)
    -> ``<stem>.png`` reconstructions in ``output_dir``, the same files the PNG route writes.
    The files are read by a pool, checked on the host (nic_rans_inspect) and decoded on the device
    ``batch_size`` at a time (read_nic groups them by latent shape); the PNG encode + write of a
    batch runs on the writer thread while the next batch is decoded (``workers=0``: inline).
    ``png_writer="device"``: the PNG files are made on the device (png_files_device) and the writer
    thread only writes them.  ``prior``: set on the model's codec first; version-2 files need the
    prior they were written under (ValueError naming the file and both ids otherwise), and their
    reconstructions are cropped on the device to the H x W they record, before either PNG writer.
    ``region`` (a pixel box (y, x, h, w)): every file is decoded to that box of its image only
    (decode_region: the segments and the latent window the box needs, not the whole frame) and
    ``<stem>.png`` holds the box, by either PNG writer; a file whose recorded H x W does not hold the
    box raises ValueError naming it.  Whole files are still read and uploaded."""
    import torch
    from concurrent.futures import ThreadPoolExecutor

    _check_png_writer(png_writer, decoder_side=True)
    if region is not None:
        region = tuple(int(v) for v in region)
        if len(region) != 4:
            raise ValueError(f"region must be a pixel box (y, x, h, w), got {region!r}")
    if prior is not None:
        _set_any_prior(model.codec, prior)
    os.makedirs(output_dir, exist_ok=True)
    model.load(checkpoint_path)
    codec = model.codec
    files = [fn for fn in sorted(os.listdir(dataset_path)) if fn.endswith(".nic")]
    serial = workers is not None and workers <= 0
    threads = _host_threads()
    png_threads = 1 if serial else (int(workers) if workers else min(16, threads))
    step = max(1, batch_size)
    with ThreadPoolExecutor(max_workers=min(8, threads)) as readers, ThreadPoolExecutor(max_workers=1) as writer:
        futures = []

        def emit(rec, stems):
            """The PNG files of the reconstructions rec, a device tensor, by the chosen writer."""
            if png_writer == "device":
                write, *args = _write_files, png_files_device(codec, rec), output_dir, stems, ".png"
            else:
                write, *args = save_imgs, rec.cpu().numpy(), output_dir, stems, png_threads  # serial: 1 thread
            while len(futures) >= WRITES_IN_FLIGHT:
                futures.pop(0).result()
            if serial:
                write(*args)
            else:
                futures.append(writer.submit(write, *args))

        chunks = [files[i:i + step] for i in range(0, len(files), step)]
        pending = [readers.map(_read_bytes, [os.path.join(dataset_path, fn) for fn in ch]) for ch in chunks[:2]]
        for k, ch in enumerate(chunks):
            datas = list(pending[k])
            pending[k] = None
            if k + 2 < len(chunks):  # two chunks of reads in flight ahead of the device
                pending.append(readers.map(_read_bytes, [os.path.join(dataset_path, fn) for fn in chunks[k + 2]]))
            names = [fn[:-4] for fn in ch]
            if region is not None:
                keys = []
                for i, data in enumerate(datas):
                    try:
                        key, size = _inspect_any(codec, i, data)
                    except ValueError as e:
                        raise ValueError(f"{dataset_path}: {ch[i]}: {e}") from None
                    if not _fits(region, size):
                        raise ValueError(f"{dataset_path}: {ch[i]}: region (y {region[0]}, x {region[1]}, {region[2]} x "
                                         f"{region[3]}) does not lie inside its {size[0]} x {size[1]} image")
                    keys.append(key)
                for i, j in _batches(keys, step):  # consecutive files that decode as one batch: one plan, one window
                    try:
                        rec = _region_of_batch(model, datas[i:j], (8 * keys[i][1], 8 * keys[i][2]), region)
                    except ValueError as e:  # the device refused an image of the batch: name its file
                        m = re.search(r"(?:file|image) (\d+)", str(e))
                        which = ch[i + int(m.group(1))] if m and i + int(m.group(1)) < j else f"files {ch[i]}..{ch[j - 1]}"
                        raise ValueError(f"{dataset_path}: {which}: {e}") from None
                    emit(rec, names[i:j])
                continue
            try:
                latents, hw = read_nic(codec, datas, sizes=True)
            except ValueError as e:
                m = re.match(r"read_nic: file (\d+): ", str(e))
                which = ch[int(m.group(1))] if m else f"files {ch[0]}..{ch[-1]}"
                raise ValueError(f"{dataset_path}: {which}: {e}") from None
            for i, j in _batches([(tuple(z.shape), size) for z, size in zip(latents, hw)], step):
                rec = model._device_call(torch.stack(latents[i:j]))
                if hw[i] != tuple(rec.shape[1:3]):  # a version-2 file's own size: the top-left corner
                    rec = rec[:, :hw[i][0], :hw[i][1]].contiguous()
                emit(rec, names[i:j])
        for f in futures:
            f.result()  # re-raise any write error
