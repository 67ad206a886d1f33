"""Frame I/O around `infer_video_depth`: the two helpers the reference's CLIs call
(/root/reference/utils/dc_utils.py:18-88 `read_video_frames`, `save_video`; same names, arguments and return values).

Not on the accelerated path. The reference decodes with decord / cv2 and encodes H.264 with
imageio-ffmpeg; none of those exist offline, so each is used when importable and otherwise replaced by what the image has:

  read_video_frames: .npy / .npz (`frames`, optional `fps`), a directory of still images, or any multi-frame file PIL opens
                     (GIF, APNG, TIFF); a video file needs decord or cv2 - except a Motion-JPEG .avi (what save_video writes,
                     webcams, `ffmpeg -c:v mjpeg`): with `device` it is decoded on the GPU (mjpeg.decode_jpeg), without it
                     it is read here (mjpeg.read_avi + PIL) when neither decord nor cv2 is importable.
  save_video       : mp4 through imageio when present, else an animated GIF (PIL) next to the requested name; with
                     codec="mjpeg" a Motion-JPEG .avi that needs neither (video_depth_anything_amd/mjpeg.py).

  read_video_blocks: read_video_frames as an iterator of blocks, for infer_video_depth_stream: with a device a Motion-JPEG .avi and
                     an .npy are read, scaled and handed over a block at a time (bounded memory).

Frames larger than `max_res` are scaled like the reference's cv2 branch (round(size * max_res / max(h, w)), bilinear, half-pixel
centres, no antialiasing = cv2.INTER_LINEAR's definition); cv2 is not here to pin that bit for bit. With a `device` the scaling is
cv2's 8-bit fixed-point arithmetic restated, on the GPU (video_depth_anything_amd/scale.py, csrc/resize_u8.hip); without one it
is rounded float bilinear on the CPU (`_resize_bilinear`), as it always was: the two differ by one level in a few percent of the
bytes (DESIGN.md 6j names this as the open inconsistency).
"""
import os

import numpy as np

IMAGE_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp")


def _resize_bilinear(frames, height, width):
    import torch
    x = torch.from_numpy(np.array(frames)).permute(0, 3, 1, 2).float()       # a copy: the source may be a read-only memory map
    y = torch.nn.functional.interpolate(x, size=(height, width), mode="bilinear", align_corners=False, antialias=False)
    return y.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()


def _decode(video_path):
    """-> (uint8 [N,H,W,3] RGB, source fps), the whole video on the host. (A Motion-JPEG .avi that is to be decoded on a device does
    not come here: read_video_blocks reads it block by block.)"""
    ext = os.path.splitext(video_path)[1].lower()
    if os.path.isdir(video_path):
        from PIL import Image
        names = sorted(n for n in os.listdir(video_path) if n.lower().endswith(IMAGE_EXT + (".npy",)))
        if not names:
            raise ValueError(f"no frames in {video_path}")
        frames = [np.load(os.path.join(video_path, n)) if n.endswith(".npy") else np.asarray(Image.open(os.path.join(video_path, n)).convert("RGB"))
                  for n in names]
        return np.stack(frames), 24.0
    if ext == ".npy":
        # memory-mapped: frames are paged in when infer_video_depth uploads the windows that read them, so a long video is never
        # held in RAM as one array (the reference's decoders return the whole video, dc_utils.py:19-69)
        return np.load(video_path, mmap_mode="r"), 24.0
    if ext == ".npz":
        z = np.load(video_path)
        return z["frames"], float(z["fps"]) if "fps" in z else 24.0
    if ext in (".gif", ".png", ".apng", ".tif", ".tiff", ".webp"):
        from PIL import Image, ImageSequence
        im = Image.open(video_path)
        dur = im.info.get("duration", 0) or 0
        frames = np.stack([np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(im)])
        return frames, (1000.0 / dur if dur > 0 else 24.0)
    try:
        from decord import VideoReader, cpu
        vid = VideoReader(video_path, ctx=cpu(0))
        return vid.get_batch(list(range(len(vid)))).asnumpy(), float(vid.get_avg_fps())
    except ImportError:
        pass
    try:
        import cv2
    except ImportError as e:
        if ext == ".avi":                                  # what save_video(codec="mjpeg") writes: the container is read here, the frames by PIL
            from video_depth_anything_amd import mjpeg
            if mjpeg.is_mjpeg_avi(video_path):
                jpegs, fps, _, _ = mjpeg.read_avi(video_path)
                return mjpeg.decode_jpegs(jpegs), fps
        raise RuntimeError(f"cannot decode {video_path}: neither decord nor cv2 is importable here; "
                           "pass frames as .npy / .npz, a directory of images or a GIF") from e
    cap = cv2.VideoCapture(video_path)
    fps = cap.get(cv2.CAP_PROP_FPS)
    out = []
    while True:
        ok, f = cap.read()
        if not ok:
            break
        out.append(cv2.cvtColor(f, cv2.COLOR_BGR2RGB))
    cap.release()
    return np.stack(out), float(fps)


def _is_mjpeg_avi(video_path):
    if os.path.splitext(video_path)[1].lower() != ".avi" or not os.path.isfile(video_path):
        return False
    from video_depth_anything_amd import mjpeg
    return mjpeg.is_mjpeg_avi(video_path)


def _fps_stride(src_fps, target_fps):
    fps = src_fps if target_fps < 0 else target_fps
    return fps, max(round(src_fps / fps), 1)


def _source_frames(video_path, process_length):
    """`_decode`'s frames (a memory map stays one) cut to `process_length` SOURCE frames, as the cv2 branch counts (dc_utils.py:57)."""
    frames, src_fps = _decode(video_path)
    if not isinstance(frames, np.ndarray):
        frames = np.asarray(frames)
    if frames.ndim != 4 or frames.shape[-1] != 3:
        raise ValueError(f"expected frames [N,H,W,3], got {frames.shape}")
    return (frames[:process_length] if process_length > 0 else frames), src_fps


def _scale(frames, max_res, device, one_block=False):
    """uint8 [m,h,w,3] under `max_res`: on `device` with cv2's 8-bit arithmetic (scale.resize_frames, csrc/resize_u8.hip), without
    one by `_resize_bilinear` as it always was (rounded float bilinear: the two differ by a level in places).
    one_block: `frames` is a block that fits the device as it is - it is uploaded here and scaled in one call; otherwise
    resize_frames stages the array through pinned buffers that it allocates per call (once per video, not once per block)."""
    from video_depth_anything_amd.scale import resize_frames, scaled_size
    h, w = frames.shape[1:3]
    H, W = scaled_size(h, w, max_res)
    if (H, W) == (h, w):
        return frames
    if device is None:
        return _resize_bilinear(frames, H, W)
    if one_block:
        import torch
        x = torch.from_numpy(frames if frames.flags.writeable else np.array(frames))      # a slice of a read-only memory map: paged in here
        return resize_frames(x.to(device), H, W).cpu().numpy()
    return resize_frames(frames, H, W, device)


def read_video_frames(video_path, process_length, target_fps=-1, max_res=-1, device=None):
    """dc_utils.py:18-70: every `stride`-th frame (stride = max(round(src_fps / fps), 1)), at most `process_length`
    frames read, frames larger than `max_res` scaled down. Returns (uint8 [N,H,W,3], fps). device (not in the reference): a cuda
    device on which a Motion-JPEG .avi is decoded (csrc/mjpeg_decode.hip) - only the frames that are kept - and on which frames
    larger than `max_res` are scaled (csrc/resize_u8.hip), block by block, whatever they were read from; None goes the way it always
    went."""
    if device is not None and _is_mjpeg_avi(video_path):
        blocks, fps = read_video_blocks(video_path, process_length, target_fps, max_res, device, block=SAVE_BLOCK)
        return np.concatenate(list(blocks)), fps
    frames, src_fps = _source_frames(video_path, process_length)
    fps, stride = _fps_stride(src_fps, target_fps)
    h, w = frames.shape[1:3]
    lazy = isinstance(frames, np.memmap) and stride == 1 and frames.dtype == np.uint8 and not (max_res > 0 and max(h, w) > max_res)
    if lazy:
        return frames, fps                            # still on disk: infer_video_depth pages in what each window reads
    return _scale(np.ascontiguousarray(frames[::stride], dtype=np.uint8), max_res, device), fps


def reads_in_blocks(video_path, device=None):
    """True for the two sources of which read_video_blocks never holds the whole: an .npy (a memory map) and, with a `device`, a
    Motion-JPEG .avi. Every other source is decoded whole anyway: a caller that needs the frames twice should keep
    read_video_frames' array instead of reading twice."""
    if os.path.isdir(video_path):
        return False
    return os.path.splitext(video_path)[1].lower() == ".npy" or (device is not None and _is_mjpeg_avi(video_path))


def _avi_blocks(video_path, process_length, stride, max_res, device, block):
    """The kept frames of a Motion-JPEG .avi, `block` at a time: decoded and scaled on the device, only the scaled block comes back."""
    import torch
    from video_depth_anything_amd import mjpeg
    from video_depth_anything_amd.scale import resize_frames, scaled_size

    def pixels(jpegs):
        try:
            x = mjpeg.decode_jpeg(jpegs, device, to_host=False)
        except mjpeg.UnsupportedJpeg:                                       # progressive, CMYK, ...: PIL reads it, the device scales it
            x = torch.from_numpy(mjpeg.decode_jpegs(jpegs)).to(device)
        if x.dim() == 3:
            x = x[..., None].expand(-1, -1, -1, 3).contiguous()
        H, W = scaled_size(x.shape[1], x.shape[2], max_res)
        return (x if (H, W) == tuple(x.shape[1:3]) else resize_frames(x, H, W)).cpu().numpy()

    jpegs = mjpeg.iter_avi(video_path, stride, process_length if process_length > 0 else None)
    next(jpegs)
    held = []
    for j in jpegs:
        held.append(j)
        if len(held) == block:
            yield pixels(held)
            held = []
    if held:
        yield pixels(held)


def read_video_blocks(video_path, process_length, target_fps=-1, max_res=-1, device=None, block=None):
    """read_video_frames as an iterator: (blocks, fps), blocks yielding uint8 [m,H,W,3] of `block` frames (default scheduler.STEP,
    a window's new frames; the last one may be shorter) whose concatenation is read_video_frames(same arguments), byte for byte. It
    is to read_video_frames what infer_video_depth_stream is to infer_video_depth: with a cuda `device`, a Motion-JPEG .avi is read
    a block at a time (dropped frames are skipped in the container, a block's JPEGs are decoded and scaled on the device and only
    the scaled block crosses to the host) and an .npy stays a memory map of which one block's source frames are paged in, uploaded
    and scaled - neither the source nor the scaled video is ever held as a whole. Every other source is decoded whole, as `_decode`
    decodes it, and cut into blocks; with device=None a block is scaled by `_resize_bilinear`, as read_video_frames scales."""
    if block is None:
        from video_depth_anything_amd.scheduler import STEP
        block = STEP
    if block < 1:
        raise ValueError(f"read_video_blocks: block must be positive, got {block}")
    if device is not None and _is_mjpeg_avi(video_path):
        from video_depth_anything_amd import mjpeg
        fps, stride = _fps_stride(next(mjpeg.iter_avi(video_path))[0], target_fps)
        return _avi_blocks(video_path, process_length, stride, max_res, device, block), fps
    frames, src_fps = _source_frames(video_path, process_length)
    fps, stride = _fps_stride(src_fps, target_fps)
    kept = frames[::stride]                                                 # a view: a memory map is not read here

    def blocks():
        for i in range(0, kept.shape[0], block):
            yield _scale(np.ascontiguousarray(kept[i:i + block], dtype=np.uint8), max_res, device, one_block=True)

    return blocks(), fps


def _inferno(u8):
    """uint8 [..] -> uint8 [..,3]: degree-6 polynomial fit of matplotlib's 'inferno', written when matplotlib could not be imported.
    It is NOT the reference's colour map: the reference indexes the 256-entry table (dc_utils.py:75-83), and this fit differs from
    (table * 255).astype(uint8) in every one of the 256 rows, by up to 9 levels. It stays as save_video's default palette, byte for
    byte (tests/test_io.py, tests/test_io_stream.py); the reference's own colours are `palette=visualize.inferno_table()`, which is
    what run.py passes. The depth values themselves (npz / exr / the returned array) never pass through either."""
    t = u8.astype(np.float32) / 255.0
    c = np.array([[0.0002189403691192265, 0.001651004631001012, -0.01948089843709184],
                  [0.1065134194856116, 0.5639564367884091, 3.932712388889277],
                  [11.60249308247187, -3.972853965665698, -15.9423941062914],
                  [-41.70399613139459, 17.43639888205313, 44.35414519872813],
                  [77.162935699427, -33.40235894210092, -81.80730925738993],
                  [-71.31942824499214, 32.62606426397723, 73.20951985803202],
                  [25.13112622477341, -12.24266895238567, -23.07032500287172]], dtype=np.float32)
    rgb = np.zeros(t.shape + (3,), dtype=np.float32)
    for k in range(6, -1, -1):
        rgb = rgb * t[..., None] + c[k]
    return (np.clip(rgb, 0, 1) * 255).astype(np.uint8)


SAVE_BLOCK = 32                                        # frames mapped to uint8 / colour at a time by save_video


def save_video(frames, output_video_path, fps=10, is_depths=False, grayscale=False, d_min=None, d_max=None, palette=None, device=None,
               codec=None, quality=90):
    """dc_utils.py:73-88. Depth is mapped through its GLOBAL min / max to uint8 (then a colour map unless `grayscale`).
    Returns the path written (the reference returns None): the .mp4 asked for, or a .gif when there is no encoder.
    Works SAVE_BLOCK frames at a time and hands each frame to the writer as it is mapped, so `frames` may be a memory map of a video
    that does not fit in RAM (run.py --stream); d_min / d_max: the global range when the caller knows it already
    (infer_video_depth_stream's depth_min / depth_max) - otherwise one block-wise pass finds it. Element by element the same
    arithmetic as mapping the whole array at once: the bytes written do not depend on the block size.
    palette / device (depth only, float32): with both None the colours are the polynomial `_inferno`, as they always were here.
    palette = uint8 [256,3] indexes that table instead - video_depth_anything_amd.visualize.inferno_table() is the reference's own
    (the contract of visualize.colorize_numpy, which adds a clamp for NaN / out-of-range pixels and treats a range
    narrower than 1e-12 as it is rather than as 1e-12). device = a cuda device maps each block on the GPU (visualize.colorize,
    csrc/visualize.hip): the same bytes as the host path for the same palette (None = inferno_table() then).
    codec: None is all of the above. "mjpeg" writes <stem>.avi instead, Motion-JPEG at `quality` (1..100) in an AVI container
    (video_depth_anything_amd.mjpeg), with no encoder library: each mapped block is coded by encode_jpeg_numpy, or
    with `device` by csrc/mjpeg.hip - the block is uploaded once, colour-mapped and coded on the device, and only the compressed
    bytes come back; the file is the same, byte for byte, either way. Source frames (is_depths=False) and gray depth take the
    same route."""
    if codec not in (None, "mjpeg"):
        raise ValueError(f"save_video: codec must be None or 'mjpeg', got {codec!r}")
    if not isinstance(frames, np.ndarray):
        frames = np.asarray(frames)
    n = frames.shape[0]
    blocks = [slice(i, min(i + SAVE_BLOCK, n)) for i in range(0, n, SAVE_BLOCK)]
    table_path = is_depths and (palette is not None or device is not None)
    if is_depths:
        if d_min is None:
            d_min = min(frames[b].min() for b in blocks)
        if d_max is None:
            d_max = max(frames[b].max() for b in blocks)
        d_min, d_max = frames.dtype.type(d_min), frames.dtype.type(d_max)
        span = max(float(d_max - d_min), 1e-12)
    if table_path:
        from video_depth_anything_amd import visualize
        to_bytes = visualize.colorize_numpy if device is None else visualize.colorize

    def mapped_block(b):
        if table_path:
            return to_bytes(frames[b], d_min, d_max, grayscale, palette, device)
        if is_depths:
            norm = ((frames[b] - d_min) / span * 255).astype(np.uint8)
            return norm if grayscale else _inferno(norm)
        return frames[b]

    def mapped():
        for b in blocks:
            for f in mapped_block(b):
                yield f

    if codec == "mjpeg":
        from video_depth_anything_amd import mjpeg
        path = os.path.splitext(output_video_path)[0] + ".avi"
        h, w = frames.shape[1:3]

        def jpegs():
            for b in blocks:
                if device is None:
                    yield from mjpeg.encode_jpeg_numpy(np.ascontiguousarray(mapped_block(b)), quality)
                else:
                    import torch
                    x = torch.from_numpy(np.array(frames[b])).to(device)                 # the only upload: depth or source frames
                    if is_depths:
                        x = visualize.colorize(x, d_min, d_max, grayscale, palette)
                    payload, lengths = mjpeg.encode_jpeg(x, quality)
                    yield from mjpeg.split_payload(mjpeg.jpeg_header(h, w, 3 if x.dim() == 4 else 1, quality), payload, lengths)

        mjpeg.write_avi(path, jpegs(), fps, w, h)
        return path

    try:
        import imageio
    except ImportError:
        imageio = None                                 # no H.264 encoder in this image: animated GIF instead (stated in the docstring)
    if imageio is not None:
        # an encoder that IS installed and fails (bad path, codec error) raises: the failure must not turn into a silent GIF
        writer = imageio.get_writer(output_video_path, fps=fps, macro_block_size=1, codec='libx264', ffmpeg_params=['-crf', '18'])
        for f in mapped():
            writer.append_data(f)
        writer.close()
        return output_video_path
    else:
        from PIL import Image
        path = os.path.splitext(output_video_path)[0] + ".gif"
        ims = (Image.fromarray(f) for f in mapped())
        next(ims).save(path, save_all=True, append_images=ims, duration=max(int(round(1000.0 / max(fps, 1e-6))), 1), loop=0)
        return path
