"""ctypes binding of the libgpujpeg C ABI (reference: libgpujpeg/gpujpeg_common.h, gpujpeg_encoder.h,
gpujpeg_decoder.h). Struct layouts mirror the reference headers field by field because they ARE the ABI.

The binding is library-agnostic: `Library(path)` loads any shared object exporting the libgpujpeg symbols.
The product library is gpujpeg_amd/lib/libgpujpeg.so (HIP kernels for gfx950); there is no CPU fallback --
loading fails loudly if it has not been built.
"""
import ctypes as C
import os

import numpy as np

MAX_COMPONENT_COUNT = 4

# enum gpujpeg_color_space (gpujpeg_type.h:85-94)
NONE, RGB, YCBCR_BT601, YCBCR_BT601_256LVLS, YCBCR_BT709, YUV = 0, 1, 2, 3, 4, 5
YCBCR_JPEG = YCBCR_BT601_256LVLS
CS_DEFAULT = -1
# enum gpujpeg_pixel_format (gpujpeg_type.h:108-134)
PIXFMT_NONE = -1
U8, P012_444, P0P1P2_444, P1020_422, P0P1P2_422, P0P1P2_420, P0123_4444 = 0, 1, 2, 3, 4, 5, 6
PIXFMT_AUTODETECT, PIXFMT_NO_ALPHA, PIXFMT_STD, PIXFMT_NATIVE = -2, -3, -4, -5
# enum gpujpeg_encoder_input_type / gpujpeg_decoder_output_type
ENCODER_INPUT_IMAGE, ENCODER_INPUT_OPENGL_TEXTURE, ENCODER_INPUT_GPU_IMAGE = 0, 1, 2
(DECODER_OUTPUT_INTERNAL_BUFFER, DECODER_OUTPUT_CUSTOM_BUFFER, DECODER_OUTPUT_OPENGL_TEXTURE,
 DECODER_OUTPUT_CUDA_BUFFER, DECODER_OUTPUT_CUSTOM_CUDA_BUFFER) = range(5)
RESTART_AUTO, RESTART_NONE = -1, 0
# Decoder.set_option(DEC_OPT_BATCH_SIZES, BATCH_SIZES_MIXED): the streams of one decode_batch_crop_resize / _tensor call may differ in image size
# (include/gpujpeg_amd_ext.h, GPUJPEG_AMD_DEC_OPT_BATCH_SIZES). RESTART_AUTO picks the interval from the image size: encode such a dataset with an
# explicit restart interval, so that its streams share one header but for the dimensions.
DEC_OPT_BATCH_SIZES = "dec_opt_batch_sizes"
BATCH_SIZES_SAME, BATCH_SIZES_MIXED = "same", "mixed"
# Decoder.set_option(DEC_OPT_BATCH_RESTARTLESS, BATCH_RESTARTLESS_ON): the batch calls take streams without restart markers (what libjpeg, PIL and
# OpenCV write) through their batched launches (GPUJPEG_AMD_DEC_OPT_BATCH_RESTARTLESS); with it a dataset needs no explicit restart interval
DEC_OPT_BATCH_RESTARTLESS = "dec_opt_batch_restartless"
BATCH_RESTARTLESS_OFF, BATCH_RESTARTLESS_ON = "off", "on"
# Decoder.set_option(DEC_OPT_PROGRESSIVE, PROGRESSIVE_ON): progressive streams (SOF2) are decoded, to the image of their baseline twin
# (GPUJPEG_AMD_DEC_OPT_PROGRESSIVE); at most PROGRESSIVE_MAX_SCANS scans. Decoder.progressive_stats() and stream_info() tell what a stream is
DEC_OPT_PROGRESSIVE = "dec_opt_progressive"
PROGRESSIVE_OFF, PROGRESSIVE_ON = "off", "on"
PROGRESSIVE_MAX_SCANS = 64
# Decoder.set_option(DEC_OPT_BATCH_PROGRESSIVE, BATCH_PROGRESSIVE_ON): with DEC_OPT_PROGRESSIVE on, the batch calls take the progressive frames that
# form a group (same size, sampling and quantisation tables) through batched launches (GPUJPEG_AMD_DEC_OPT_BATCH_PROGRESSIVE);
# Decoder.progressive_batch_stats() tells what they took
DEC_OPT_BATCH_PROGRESSIVE = "dec_opt_batch_progressive"
BATCH_PROGRESSIVE_OFF, BATCH_PROGRESSIVE_ON = "off", "on"
# Decoder.set_option(DEC_OPT_BATCH_HEADERS, BATCH_HEADERS_ANY): next to DEC_OPT_BATCH_SIZES = mixed, the streams of one crop-and-resize call may also
# differ in quantisation tables, Huffman tables and marker segments and still share the batched launches (GPUJPEG_AMD_DEC_OPT_BATCH_HEADERS);
# Decoder.batch_header_stats() tells what the call's family was
DEC_OPT_BATCH_HEADERS = "dec_opt_batch_headers"
BATCH_HEADERS_SAME, BATCH_HEADERS_ANY = "same", "any"
# encoder option of the MI355X build (gpujpeg_amd_ext.h: GPUJPEG_AMD_ENC_OPT_HUFFMAN): Annex K.3 tables, or tables built per frame
ENC_OPT_HUFFMAN = "enc_opt_huffman"
ENC_HUFFMAN_STANDARD, ENC_HUFFMAN_OPTIMAL = "standard", "optimal"


def MK_SUBSAMPLING(*f):
    f = list(f) + [0] * (8 - len(f))
    v = 0
    for x in f:
        v = (v << 4) | x
    return v


SUBSAMPLING_444 = MK_SUBSAMPLING(1, 1, 1, 1, 1, 1)
SUBSAMPLING_422 = MK_SUBSAMPLING(2, 1, 1, 1, 1, 1)
SUBSAMPLING_420 = MK_SUBSAMPLING(2, 2, 1, 1, 1, 1)
SUBSAMPLING_4444 = MK_SUBSAMPLING(1, 1, 1, 1, 1, 1, 1, 1)
SUBSAMPLING_400 = MK_SUBSAMPLING(1, 1)


class SamplingFactor(C.Structure):
    _fields_ = [("horizontal", C.c_uint8), ("vertical", C.c_uint8)]


class Parameters(C.Structure):  # struct gpujpeg_parameters, gpujpeg_common.h:176-215
    _fields_ = [("verbose", C.c_int), ("perf_stats", C.c_int), ("quality", C.c_int), ("restart_interval", C.c_int),
                ("interleaved", C.c_int), ("segment_info", C.c_int), ("comp_count", C.c_int),
                ("sampling_factor", SamplingFactor * MAX_COMPONENT_COUNT), ("color_space_internal", C.c_int)]


class ImageParameters(C.Structure):  # struct gpujpeg_image_parameters, gpujpeg_common.h:283-294
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("color_space", C.c_int), ("pixel_format", C.c_int),
                ("width_padding", C.c_int)]


class EncoderInput(C.Structure):  # gpujpeg_encoder.h:57-67
    _fields_ = [("type", C.c_int), ("image", C.c_void_p), ("texture", C.c_void_p)]


class DecoderOutput(C.Structure):  # gpujpeg_decoder.h:66-84
    _fields_ = [("type", C.c_int), ("data", C.c_void_p), ("data_size", C.c_size_t), ("param_image", ImageParameters),
                ("texture", C.c_void_p), ("metadata", C.c_void_p)]


class DecoderInitParameters(C.Structure):  # gpujpeg_decoder.h:90-97
    _fields_ = [("stream", C.c_void_p), ("verbose", C.c_int), ("perf_stats", C.c_bool), ("ff_cs_itu601_is_709", C.c_bool)]


class DurationStats(C.Structure):  # gpujpeg_common.h:352-362
    _fields_ = [(n, C.c_double) for n in ("duration_memory_to", "duration_memory_from", "duration_memory_map",
                                          "duration_memory_unmap", "duration_preprocessor", "duration_dct_quantization",
                                          "duration_huffman_coder", "duration_stream", "duration_in_gpu")]


class _ImageInfoFields(C.Structure):
    _fields_ = [("param_image", ImageParameters), ("param", Parameters), ("segment_count", C.c_int),
                ("header_type", C.c_int), ("comment", C.c_char_p), ("metadata", C.c_uint8 * 8)]


class ImageInfo(C.Union):  # gpujpeg_decoder.h:270-283 (512-byte union)
    _anonymous_ = ("f",)
    _fields_ = [("f", _ImageInfoFields), ("reserved", C.c_char * 512)]


TENSOR_F32, TENSOR_F16, TENSOR_BF16 = 0, 1, 2  # gpujpeg_amd_ext.h: GPUJPEG_AMD_TENSOR_*
TENSOR_CHW, TENSOR_HWC = 0, 1
TENSOR_ELSIZE = {TENSOR_F32: 4, TENSOR_F16: 2, TENSOR_BF16: 2}
TENSOR_NUMPY = {TENSOR_F32: np.float32, TENSOR_F16: np.float16, TENSOR_BF16: np.uint16}  # (bfloat16: the bit patterns)


class TensorFormat(C.Structure):  # gpujpeg_amd_ext.h: struct gpujpeg_amd_tensor_format (40 bytes; scale / bias [3] reserved)
    _fields_ = [("dtype", C.c_int), ("layout", C.c_int), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


def tensor_format(dtype, layout, scale, bias):
    """a TensorFormat from an element type, a layout and up to three scales and biases (a scalar: the same for every channel)"""
    fmt = TensorFormat()
    fmt.dtype, fmt.layout = int(dtype), int(layout)
    for name, values in (("scale", scale), ("bias", bias)):
        values = [float(values)] * 3 if np.isscalar(values) else [float(v) for v in values]
        if not 1 <= len(values) <= 4:
            raise ValueError(f"{name}: one value per channel")
        for c, v in enumerate(values):
            getattr(fmt, name)[c] = v
    return fmt


def tensor_element(lib, fmt, c, v):
    """gpujpeg_amd_host_tensor_element (host only, lib: a Library): the bits decode_batch_crop_resize_tensor stores for byte v of channel c"""
    return int(lib.L.gpujpeg_amd_host_tensor_element(C.byref(fmt), int(c), int(v)))


PRODUCT_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libgpujpeg.so")


class Library:
    """Thin typed handle on a libgpujpeg shared object."""

    def __init__(self, path=None):
        path = path or PRODUCT_LIB
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                    "(the HIP library is mandatory, there is no CPU fallback)")
        self.path = path
        L = self.L = C.CDLL(path, mode=C.RTLD_LOCAL)
        vp = C.c_void_p
        L.gpujpeg_set_default_parameters.argtypes = [C.POINTER(Parameters)]
        L.gpujpeg_image_set_default_parameters.argtypes = [C.POINTER(ImageParameters)]
        L.gpujpeg_parameters_chroma_subsampling.argtypes = [C.POINTER(Parameters), C.c_uint32]
        L.gpujpeg_image_calculate_size.restype = C.c_size_t
        L.gpujpeg_image_calculate_size.argtypes = [C.POINTER(ImageParameters)]
        L.gpujpeg_init_device.argtypes = [C.c_int, C.c_int]
        L.gpujpeg_encoder_create.restype = vp
        L.gpujpeg_encoder_create.argtypes = [vp]
        L.gpujpeg_encoder_destroy.argtypes = [vp]
        L.gpujpeg_encoder_encode.argtypes = [vp, C.POINTER(Parameters), C.POINTER(ImageParameters), C.POINTER(EncoderInput),
                                             C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
        L.gpujpeg_encoder_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
        L.gpujpeg_encoder_suggest_restart_interval.argtypes = [C.POINTER(ImageParameters), C.c_uint32, C.c_bool, C.c_int]
        L.gpujpeg_encoder_get_stats.argtypes = [vp, C.POINTER(DurationStats)]
        L.gpujpeg_decoder_create.restype = vp
        L.gpujpeg_decoder_create.argtypes = [vp]
        L.gpujpeg_decoder_destroy.argtypes = [vp]
        L.gpujpeg_decoder_init.argtypes = [vp, C.POINTER(Parameters), C.POINTER(ImageParameters)]
        L.gpujpeg_decoder_decode.argtypes = [vp, vp, C.c_size_t, C.POINTER(DecoderOutput)]
        L.gpujpeg_decoder_set_output_format.argtypes = [vp, C.c_int, C.c_int]
        L.gpujpeg_decoder_set_output_format.restype = None
        L.gpujpeg_decoder_get_stats.argtypes = [vp, C.POINTER(DurationStats)]
        L.gpujpeg_decoder_get_image_info.argtypes = [vp, C.c_size_t, C.POINTER(ImageParameters), C.POINTER(Parameters), C.POINTER(C.c_int)]
        L.gpujpeg_decoder_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
        L.gpujpeg_version.restype = C.c_int
        if hasattr(L, "gpujpeg_amd_encoder_read_coefficients"):  # MI355X extensions (include/gpujpeg_amd_ext.h)
            for n in ("gpujpeg_amd_encoder_read_coefficients", "gpujpeg_amd_decoder_read_coefficients"):
                getattr(L, n).restype = C.c_size_t
                getattr(L, n).argtypes = [vp, C.POINTER(C.c_int16), C.c_size_t]
            for n in ("gpujpeg_amd_encoder_read_planes", "gpujpeg_amd_decoder_read_planes"):
                getattr(L, n).restype = C.c_size_t
                getattr(L, n).argtypes = [vp, C.POINTER(C.c_uint8), C.c_size_t]
            for n in ("gpujpeg_amd_encoder_get_kernel_times", "gpujpeg_amd_decoder_get_kernel_times"):
                getattr(L, n).argtypes = [vp, C.POINTER(C.c_float)]
            for n in ("gpujpeg_amd_encoder_set_fused", "gpujpeg_amd_decoder_set_fused", "gpujpeg_amd_decoder_keep_coefficients", "gpujpeg_amd_encoder_keep_coefficients"):
                getattr(L, n).restype = None
                getattr(L, n).argtypes = [vp, C.c_int]
        if hasattr(L, "gpujpeg_amd_encoder_encode_batch"):  # frame batches (include/gpujpeg_amd_ext.h)
            L.gpujpeg_amd_encoder_encode_batch.argtypes = [vp, C.POINTER(Parameters), C.POINTER(ImageParameters), vp, C.c_size_t, C.c_int,
                                                           C.POINTER(vp), C.POINTER(C.c_size_t)]
        for n in ("gpujpeg_amd_encoder_set_batch_chunk", "gpujpeg_amd_decoder_set_batch_chunk"):
            if hasattr(L, n):
                getattr(L, n).restype = None
                getattr(L, n).argtypes = [vp, C.c_int]
        for n in ("gpujpeg_amd_encoder_last_batch", "gpujpeg_amd_decoder_last_batch"):
            if hasattr(L, n):
                getattr(L, n).argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        if hasattr(L, "gpujpeg_amd_encoder_encode_batch_ptrs"):
            L.gpujpeg_amd_encoder_encode_batch_ptrs.argtypes = [vp, C.POINTER(Parameters), C.POINTER(ImageParameters), C.POINTER(vp), C.c_int,
                                                                C.POINTER(vp), C.POINTER(C.c_size_t)]
            L.gpujpeg_amd_decoder_decode_batch_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_int, C.POINTER(vp), C.c_size_t,
                                                                C.POINTER(ImageParameters)]
        if hasattr(L, "gpujpeg_amd_decoder_decode_batch"):
            L.gpujpeg_amd_decoder_decode_batch.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int, vp, C.c_size_t, C.POINTER(ImageParameters)]
        if hasattr(L, "gpujpeg_amd_decoder_decode_batch_regions"):
            L.gpujpeg_amd_decoder_decode_batch_regions.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int,
                                                                   vp, C.c_size_t, C.POINTER(ImageParameters)]
        if hasattr(L, "gpujpeg_amd_decoder_decode_batch_crop_resize"):
            L.gpujpeg_amd_decoder_decode_batch_crop_resize.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_int),
                                                                       C.POINTER(C.c_uint8), C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(ImageParameters)]
        if hasattr(L, "gpujpeg_amd_decoder_decode_batch_crop_resize_tensor"):
            L.gpujpeg_amd_decoder_decode_batch_crop_resize_tensor.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_int),
                                                                              C.POINTER(C.c_uint8), C.c_int, C.c_int, C.POINTER(TensorFormat), vp, C.c_size_t,
                                                                              C.POINTER(ImageParameters)]
            L.gpujpeg_amd_host_tensor_element.restype = C.c_uint32
            L.gpujpeg_amd_host_tensor_element.argtypes = [C.POINTER(TensorFormat), C.c_int, C.c_int]
        if hasattr(L, "gpujpeg_amd_host_crop_resize_plan"):
            L.gpujpeg_amd_host_crop_resize_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
            L.gpujpeg_amd_decoder_get_prescales.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int]
        if hasattr(L, "gpujpeg_amd_host_orientation_plan"):
            L.gpujpeg_amd_host_orientation_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
            L.gpujpeg_amd_host_stream_orientation.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        if hasattr(L, "gpujpeg_amd_host_resize_weights"):
            L.gpujpeg_amd_host_resize_weights.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.c_int,
                                                          C.POINTER(C.c_uint64)]

    # ---- developer settings (include/gpujpeg_amd_ext.h: gpujpeg_amd_tuning) ----
    def tuning(self, setting):
        """"NAME=VALUE" / "NAME" for the coders created from now on, None forgets every setting. True when the library took it
        (False: unknown name, or a library without the call -- the reference builds)."""
        if not hasattr(self.L, "gpujpeg_amd_tuning"):
            return False
        self.L.gpujpeg_amd_tuning.argtypes = [C.c_char_p]
        return self.L.gpujpeg_amd_tuning(None if setting is None else setting.encode()) == 0

    def tuning_names(self):
        if not hasattr(self.L, "gpujpeg_amd_tuning_names"):
            return []
        self.L.gpujpeg_amd_tuning_names.restype = C.POINTER(C.c_char_p)
        arr, out, i = self.L.gpujpeg_amd_tuning_names(), [], 0
        while arr[i]:
            out.append(arr[i].decode())
            i += 1
        return out

    # ---- parameter helpers ----
    def default_parameters(self):
        p = Parameters()
        self.L.gpujpeg_set_default_parameters(C.byref(p))
        return p

    def default_image_parameters(self):
        p = ImageParameters()
        self.L.gpujpeg_image_set_default_parameters(C.byref(p))
        return p

    def image_size(self, param_image):
        return self.L.gpujpeg_image_calculate_size(C.byref(param_image))


def crop_resize_plan(lib, image_w, image_h, all_components_1x1, rect, out_w, out_h, max_scale):
    """gpujpeg_amd_host_crop_resize_plan (host only, lib: a Library): what dec_opt_resize_prescale = 1/max_scale gives one frame of a crop-and-resize
    call -- rect = (x, y, w, h) of an image_w x image_h image resampled to out_w x out_h -> (s, x', y', w', h'), or None where the call would refuse"""
    out = (C.c_int * 5)()
    r4 = (C.c_int * 4)(*[int(v) for v in rect])
    rc = lib.L.gpujpeg_amd_host_crop_resize_plan(int(image_w), int(image_h), int(bool(all_components_1x1)), r4, int(out_w), int(out_h), int(max_scale), out)
    return tuple(out) if rc == 0 else None


def orientation_plan(lib, image_w, image_h, rotation, flip, rect, out_w, out_h, mirror=False):
    """gpujpeg_amd_host_orientation_plan (host only, lib: a Library): rect = (x, y, w, h) in the display image of an image_w x image_h stored image turned
    by `rotation` quarter turns clockwise and then mirrored if `flip`, wanted as out_w x out_h display-oriented pixels -> (x', y', w', h', OW', OH', bits):
    the rectangle and output size to hand to decode_batch_crop_resize, and bits = 1 reverse the columns of its frame | 2 reverse its rows | 4 swap the
    axes; None for a rectangle outside the display image or an output size outside 1 .. 16384"""
    out = (C.c_int * 8)()
    r4 = (C.c_int * 4)(*[int(v) for v in rect])
    rc = lib.L.gpujpeg_amd_host_orientation_plan(int(image_w), int(image_h), int(rotation), int(bool(flip)), r4, int(out_w), int(out_h), int(bool(mirror)), out)
    return tuple(out)[:7] if rc == 0 else None


def stream_orientation(lib, jpeg):
    """gpujpeg_amd_host_stream_orientation (host only, lib: a Library): (set 0 / 1, rotation, flip, display width, display height) as the reader finds them
    in the stream's headers (Exif APP1 or SPIFF); None when the headers cannot be parsed"""
    a = np.ascontiguousarray(jpeg, np.uint8)
    out = (C.c_int * 5)()
    return tuple(out) if lib.L.gpujpeg_amd_host_stream_orientation(a.ctypes.data, a.size, out) == 0 else None


def stream_info(lib, jpeg):
    """gpujpeg_amd_host_stream_info (host only, lib: a Library): (width, height, components, progressive 0 / 1, scans, dependency levels, restart
    interval, 0 for a valid scan script or 1 + the first offending scan) of a baseline or progressive stream; None when its headers cannot be parsed"""
    a = np.ascontiguousarray(jpeg, np.uint8)
    out = (C.c_int * 8)()
    f = lib.L.gpujpeg_amd_host_stream_info
    f.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
    return tuple(out) if f(a.ctypes.data, a.size, out) == 0 else None


def resize_weights(lib, n_src, n_out, i, capacity=None):
    """gpujpeg_amd_host_resize_weights (host only, lib: a Library): the taps dec_opt_resize_filter = antialias gives output sample i along an axis of
    n_src source samples resampled to n_out -> (first, [weights], sum); None where the call would refuse. capacity: room offered for the weights
    (default: enough); too little raises ValueError with the count needed"""
    first, count, total = C.c_int(), C.c_int(), C.c_uint64()
    if lib.L.gpujpeg_amd_host_resize_weights(int(n_src), int(n_out), int(i), C.byref(first), C.byref(count), None, 0, C.byref(total)) != 0:
        return None
    cap = count.value if capacity is None else int(capacity)
    w = (C.c_uint32 * max(cap, 1))()
    rc = lib.L.gpujpeg_amd_host_resize_weights(int(n_src), int(n_out), int(i), C.byref(first), C.byref(count), w, cap, C.byref(total))
    if rc == -2:
        raise ValueError(f"capacity {cap} < {count.value} taps")
    return (first.value, [int(v) for v in w[:count.value]], int(total.value)) if rc == 0 else None


def apply_environment_settings(lib, environ=None):
    """DEVELOPER AID for tests and measurement tools: hand the developer settings named in the environment (GJ_DEC_TOKENS=1, GJ_ENC_TAIL=0, ...;
    INTEGRATION.md) to the library through gpujpeg_amd_tuning -- the library itself never reads the environment. Coders created afterwards
    take them. No-op for libraries without the call (the reference builds under oracle/_ref)."""
    import os
    env = os.environ if environ is None else environ
    if not lib.tuning(None):
        return
    for name in lib.tuning_names():
        if name in env:
            lib.tuning(f"{name}={env[name]}")


class Encoder:
    """Mirror of the reference encoder object: gpujpeg_encoder_create/encode/destroy (gpujpeg_encoder.h:118-176)."""

    def __init__(self, lib, stream=None):
        self.lib = lib
        self.h = lib.L.gpujpeg_encoder_create(stream)
        if not self.h:
            raise RuntimeError("gpujpeg_encoder_create failed")

    def set_option(self, opt, val):
        return self.lib.L.gpujpeg_encoder_set_option(self.h, opt.encode(), val.encode())

    def encode(self, param, param_image, image, gpu=False):
        """image: numpy uint8 array (host) or an integer device pointer when gpu=True. Returns numpy uint8 copy."""
        ptr, n = self.encode_noclone(param, param_image, image, gpu)
        return np.ctypeslib.as_array(ptr, shape=(n,)).copy()

    def encode_noclone(self, param, param_image, image, gpu=False):
        inp = EncoderInput()
        if gpu:
            inp.type, inp.image = ENCODER_INPUT_GPU_IMAGE, int(image)
        else:
            image = np.ascontiguousarray(image, np.uint8)
            self._keep = image
            inp.type, inp.image = ENCODER_INPUT_IMAGE, image.ctypes.data
        out, size = C.POINTER(C.c_uint8)(), C.c_size_t(0)
        rc = self.lib.L.gpujpeg_encoder_encode(self.h, C.byref(param), C.byref(param_image), C.byref(inp), C.byref(out), C.byref(size))
        if rc != 0:
            raise RuntimeError(f"gpujpeg_encoder_encode failed ({rc})")
        return out, size.value

    def encode_batch_noclone(self, param, param_image, frames, count, stride=None, gpu=False):
        """gpujpeg_amd_encoder_encode_batch: `count` frames of one geometry behind one set of launches. frames: numpy uint8 array holding
        the frames back to back (host), or an integer device pointer when gpu=True; stride: bytes between two frames (default: a frame).
        Returns ([pointer], [size]) of the streams -- device pointers with enc_opt_out=device, host pointers otherwise."""
        if gpu:
            base = int(frames)
        else:
            frames = np.ascontiguousarray(frames, np.uint8)
            self._keep = frames
            base = frames.ctypes.data
        if stride is None:
            stride = self.lib.image_size(param_image)
        ptrs, sizes = (C.c_void_p * count)(), (C.c_size_t * count)()
        rc = self.lib.L.gpujpeg_amd_encoder_encode_batch(self.h, C.byref(param), C.byref(param_image), base, stride, count, ptrs, sizes)
        if rc != 0:
            raise RuntimeError(f"gpujpeg_amd_encoder_encode_batch failed ({rc})")
        return [int(p or 0) for p in ptrs], [int(n) for n in sizes]

    def set_batch_chunk(self, frames):
        self.lib.L.gpujpeg_amd_encoder_set_batch_chunk(self.h, int(frames))

    def last_batch(self):
        """(frames coded by the batched launches, frames coded one by one) of the last encode_batch call"""
        a, b = C.c_int(0), C.c_int(0)
        self.lib.L.gpujpeg_amd_encoder_last_batch(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def encode_batch_ptrs(self, param, param_image, frames):
        """gpujpeg_amd_encoder_encode_batch_ptrs: frames = list of numpy uint8 arrays (host) and / or integer device pointers, one buffer per frame.
        Returns the streams as numpy copies (encoder output in host memory, the default)."""
        n = len(frames)
        keep = [np.ascontiguousarray(f, np.uint8) if not isinstance(f, int) else f for f in frames]
        self._keep = keep
        fp = (C.c_void_p * n)(*[f if isinstance(f, int) else f.ctypes.data for f in keep])
        ptrs, sizes = (C.c_void_p * n)(), (C.c_size_t * n)()
        rc = self.lib.L.gpujpeg_amd_encoder_encode_batch_ptrs(self.h, C.byref(param), C.byref(param_image), fp, n, ptrs, sizes)
        if rc != 0:
            raise RuntimeError(f"gpujpeg_amd_encoder_encode_batch_ptrs failed ({rc})")
        return [np.frombuffer((C.c_uint8 * int(s)).from_address(int(p)), np.uint8).copy() for p, s in zip(ptrs, sizes)]

    def encode_batch(self, param, param_image, frames, count, stride=None):
        """host frames in, list of numpy uint8 copies of the streams out (encoder output in host memory, the default)"""
        ptrs, sizes = self.encode_batch_noclone(param, param_image, frames, count, stride)
        return [np.frombuffer((C.c_uint8 * n).from_address(p), np.uint8).copy() for p, n in zip(ptrs, sizes)]

    def stats(self):
        s = DurationStats()
        self.lib.L.gpujpeg_encoder_get_stats(self.h, C.byref(s))
        return s

    def set_fused(self, enabled):
        self.lib.L.gpujpeg_amd_encoder_set_fused(self.h, int(enabled))

    def keep_coefficients(self, enabled=True):
        """Leave the quantised coefficients of the following encode calls in HBM (for coefficients())."""
        self.lib.L.gpujpeg_amd_encoder_keep_coefficients(self.h, int(enabled))

    def kernel_times(self, count=5):
        """durations of the last perf_stats call's kernels; count=6 adds [5] k_huffman_count (optimal tables)"""
        ms = (C.c_float * 8)()
        if self.lib.L.gpujpeg_amd_encoder_get_kernel_times(self.h, ms) != 0:
            return None
        return list(ms)[:count]

    def coefficients(self, count):
        a = np.empty(count, np.int16)
        n = self.lib.L.gpujpeg_amd_encoder_read_coefficients(self.h, a.ctypes.data_as(C.POINTER(C.c_int16)), count)
        return a[:n]

    def planes(self, count):
        a = np.empty(count, np.uint8)
        n = self.lib.L.gpujpeg_amd_encoder_read_planes(self.h, a.ctypes.data_as(C.POINTER(C.c_uint8)), count)
        return a[:n]

    def close(self):
        if self.h:
            self.lib.L.gpujpeg_encoder_destroy(self.h)
            self.h = None

    __del__ = close


class Decoder:
    """Mirror of the reference decoder object: gpujpeg_decoder_create/decode/destroy (gpujpeg_decoder.h:153-202)."""

    def __init__(self, lib, stream=None):
        self.lib = lib
        self.h = lib.L.gpujpeg_decoder_create(stream)
        if not self.h:
            raise RuntimeError("gpujpeg_decoder_create failed")

    def set_output_format(self, color_space, pixel_format):
        self.lib.L.gpujpeg_decoder_set_output_format(self.h, color_space, pixel_format)

    def set_option(self, opt, val):
        """gpujpeg_decoder_set_option, e.g. ("dec_opt_scale", "1/4"): the decode calls that follow return the reduced image (their
        ImageParameters and sizes are the reduced image's), or ("dec_opt_region", "x,y,w,h"): they return the w x h pixels at (x, y) of the
        stream's image ("full": the whole image again; a region that does not fit the stream or the output format's sampling grid is refused by
        the decode call). Returns the library's code (0 = accepted)."""
        return self.lib.L.gpujpeg_decoder_set_option(self.h, opt.encode(), val.encode())

    def init(self, param, param_image):
        return self.lib.L.gpujpeg_decoder_init(self.h, C.byref(param), C.byref(param_image))

    def decode(self, jpeg, device_out=None):
        """jpeg: numpy uint8 array. Returns (numpy uint8 copy of pixels, ImageParameters); with device_out
        (integer device pointer) decodes into that buffer and returns (None, ImageParameters)."""
        jpeg = np.ascontiguousarray(jpeg, np.uint8)
        out = DecoderOutput()
        if device_out is not None:
            out.type, out.data = DECODER_OUTPUT_CUSTOM_CUDA_BUFFER, int(device_out)
        else:
            out.type = DECODER_OUTPUT_INTERNAL_BUFFER
        rc = self.lib.L.gpujpeg_decoder_decode(self.h, jpeg.ctypes.data, jpeg.size, C.byref(out))
        if rc != 0:
            raise RuntimeError(f"gpujpeg_decoder_decode failed ({rc})")
        if device_out is not None:
            return None, out.param_image
        buf = (C.c_uint8 * out.data_size).from_address(out.data)
        return np.frombuffer(buf, np.uint8).copy(), out.param_image

    def set_batch_chunk(self, frames):
        self.lib.L.gpujpeg_amd_decoder_set_batch_chunk(self.h, int(frames))

    def last_batch(self):
        """(frames decoded by the batched launches, frames decoded one by one) of the last decode_batch call"""
        a, b = C.c_int(0), C.c_int(0)
        self.lib.L.gpujpeg_amd_decoder_last_batch(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def decode_batch_ptrs(self, streams, frame_bytes):
        """gpujpeg_amd_decoder_decode_batch_ptrs: one buffer per stream and per decoded frame (host memory here). Returns (list of pixel arrays, ImageParameters)."""
        n = len(streams)
        keep = [np.ascontiguousarray(s, np.uint8) for s in streams]
        outs = [np.empty(frame_bytes, np.uint8) for _ in range(n)]
        sp = (C.c_void_p * n)(*[s.ctypes.data for s in keep])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        csz = (C.c_size_t * n)(*[s.size for s in keep])
        pi = ImageParameters()
        rc = self.lib.L.gpujpeg_amd_decoder_decode_batch_ptrs(self.h, sp, csz, n, op, frame_bytes, C.byref(pi))
        if rc != 0:
            raise RuntimeError(f"gpujpeg_amd_decoder_decode_batch_ptrs failed ({rc})")
        raw = self.lib.image_size(pi)
        return [o[:raw] for o in outs], pi

    def decode_batch(self, streams, device_out=None, out_stride=None, device_in=None, in_stride=None, sizes=None, frame_bytes=None):
        """gpujpeg_amd_decoder_decode_batch: streams with one header behind one set of launches. streams: list of numpy uint8 arrays (host;
        packed into one buffer here), or device_in = integer device pointer of stream 0 with in_stride and sizes. Pixels go to device_out
        (integer device pointer, frames out_stride apart) or come back as a list of numpy arrays. Returns (pixels or None, ImageParameters)."""
        if device_in is None:
            sizes = [int(x.size) for x in streams]
            in_stride = (max(sizes) + 64 + 15) & ~15
            buf = np.zeros(in_stride * len(sizes), np.uint8)
            for i, x in enumerate(streams):
                buf[i * in_stride:i * in_stride + x.size] = x
            self._keep = buf
            base = buf.ctypes.data
        else:
            base = int(device_in)
        n = len(sizes)
        csz = (C.c_size_t * n)(*sizes)
        pi = ImageParameters()
        if device_out is not None:
            rc = self.lib.L.gpujpeg_amd_decoder_decode_batch(self.h, base, in_stride, csz, n, int(device_out), out_stride, C.byref(pi))
            if rc != 0:
                raise RuntimeError(f"gpujpeg_amd_decoder_decode_batch failed ({rc})")
            return None, pi
        # host output: the frame size is not known before the first stream has been parsed -- ask the library (streams in host memory),
        # or take the caller's word (device streams: frame_bytes = room per decoded frame)
        if device_in is not None:
            if not frame_bytes:
                raise ValueError("decode_batch(device_in=..., device_out=None) needs frame_bytes: the size of a decoded frame is not known "
                                 "before a stream has been parsed, and the streams are in device memory")
            bound = int(frame_bytes)
        else:
            # (gpujpeg_amd_host_stream_info takes progressive streams too, which gpujpeg_decoder_get_image_info refuses)
            first = np.ascontiguousarray(streams[0])
            if hasattr(self.lib.L, "gpujpeg_amd_host_stream_info"):
                info = stream_info(self.lib, first)
                if info is None:
                    raise RuntimeError("gpujpeg_amd_host_stream_info failed")
                w0, h0 = info[0], info[1]
            else:
                pi0, p0 = ImageParameters(), Parameters()
                if self.lib.L.gpujpeg_decoder_get_image_info(first.ctypes.data_as(C.c_void_p), first.size, C.byref(pi0), C.byref(p0), None) != 0:
                    raise RuntimeError("gpujpeg_decoder_get_image_info failed")
                w0, h0 = pi0.width, pi0.height
            bound = max(int(w0) * int(h0) * 4 + 4096, 1)  # (the library checks the real frame size against the stride)
        out = np.empty(bound * n, np.uint8)
        rc = self.lib.L.gpujpeg_amd_decoder_decode_batch(self.h, base, in_stride, csz, n, out.ctypes.data, bound, C.byref(pi))
        if rc != 0:
            raise RuntimeError(f"gpujpeg_amd_decoder_decode_batch failed ({rc})")
        raw = self.lib.image_size(pi)
        return [out[i * bound:i * bound + raw].copy() for i in range(n)], pi

    def decode_batch_regions(self, streams, origins, width, height, device_out=None, out_stride=None, device_in=None, in_stride=None, sizes=None):
        """gpujpeg_amd_decoder_decode_batch_regions: decode_batch with one crop per frame -- frame f is the width x height pixels at origins[f] = (x, y)
        of stream f's image. streams / device_in, in_stride, sizes and device_out, out_stride as for decode_batch; without device_out the crops come
        back as a list of numpy arrays. Returns (pixels or None, ImageParameters)."""
        if device_in is None:
            sizes = [int(x.size) for x in streams]
            in_stride = (max(sizes) + 64 + 15) & ~15
            buf = np.zeros(in_stride * len(sizes), np.uint8)
            for i, x in enumerate(streams):
                buf[i * in_stride:i * in_stride + x.size] = x
            self._keep = buf
            base = buf.ctypes.data
        else:
            base = int(device_in)
        n = len(sizes)
        if len(origins) != n:
            raise ValueError("decode_batch_regions needs one origin per stream")
        csz = (C.c_size_t * n)(*sizes)
        org = (C.c_int * (2 * n))(*[int(v) for xy in origins for v in xy])
        pi = ImageParameters()
        call = self.lib.L.gpujpeg_amd_decoder_decode_batch_regions
        if device_out is not None:
            rc = call(self.h, base, in_stride, csz, n, org, int(width), int(height), int(device_out), out_stride, C.byref(pi))
            if rc != 0:
                raise RuntimeError(f"gpujpeg_amd_decoder_decode_batch_regions failed ({rc})")
            return None, pi
        bound = max(int(width), 1) * max(int(height), 1) * 4 + 4096 * max(int(height), 1)  # (room for any format and line alignment up to 4 KiB)
        out = np.empty(bound * n, np.uint8)
        rc = call(self.h, base, in_stride, csz, n, org, int(width), int(height), out.ctypes.data, bound, C.byref(pi))
        if rc != 0:
            raise RuntimeError(f"gpujpeg_amd_decoder_decode_batch_regions failed ({rc})")
        raw = self.lib.image_size(pi)
        return [out[i * bound:i * bound + raw].copy() for i in range(n)], pi

    def decode_batch_crop_resize(self, streams, rects, out_width, out_height, mirror=None, device_out=None, out_stride=None, device_in=None, in_stride=None,
                                 sizes=None):
        """gpujpeg_amd_decoder_decode_batch_crop_resize: decode_batch with one rectangle per frame, each of its own size -- frame f is the
        rects[f] = (x, y, w, h) pixels of stream f's image resampled bilinearly to out_width x out_height and, where mirror[f] is set, mirrored
        horizontally (the definition: include/gpujpeg_amd_ext.h; set_option("dec_opt_resize_filter", "antialias") makes the resample the antialiased
        triangle filter, whose taps resize_weights() returns). streams / device_in, in_stride, sizes and device_out, out_stride as for decode_batch;
        without device_out the frames come back as a list of numpy arrays. Returns (pixels or None, ImageParameters)."""
        if not hasattr(self.lib.L, "gpujpeg_amd_decoder_decode_batch_crop_resize"):
            raise RuntimeError("this library has no gpujpeg_amd_decoder_decode_batch_crop_resize")
        if device_in is None:
            sizes = [int(x.size) for x in streams]
            in_stride = (max(sizes) + 64 + 15) & ~15
            buf = np.zeros(in_stride * len(sizes), np.uint8)
            for i, x in enumerate(streams):
                buf[i * in_stride:i * in_stride + x.size] = x
            self._keep = buf
            base = buf.ctypes.data
        else:
            base = int(device_in)
        n = len(sizes)
        if len(rects) != n or (mirror is not None and len(mirror) != n):
            raise ValueError("decode_batch_crop_resize needs one rectangle (and, with mirror, one flag) per stream")
        csz = (C.c_size_t * n)(*sizes)
        rc4 = (C.c_int * (4 * n))(*[int(v) for r in rects for v in r])
        mir = None if mirror is None else (C.c_uint8 * n)(*[1 if m else 0 for m in mirror])
        pi = ImageParameters()
        call = self.lib.L.gpujpeg_amd_decoder_decode_batch_crop_resize
        if device_out is not None:
            rc = call(self.h, base, in_stride, csz, n, rc4, mir, int(out_width), int(out_height), int(device_out), out_stride, C.byref(pi))
            if rc != 0:
                raise RuntimeError(f"gpujpeg_amd_decoder_decode_batch_crop_resize failed ({rc})")
            return None, pi
        ow, oh = min(max(int(out_width), 1), 16384), min(max(int(out_height), 1), 16384)
        bound = ow * oh * 4 + 4096 * oh  # (room for any format and line alignment up to 4 KiB)
        out = np.empty(bound * n, np.uint8)
        rc = call(self.h, base, in_stride, csz, n, rc4, mir, int(out_width), int(out_height), out.ctypes.data, bound, C.byref(pi))
        if rc != 0:
            raise RuntimeError(f"gpujpeg_amd_decoder_decode_batch_crop_resize failed ({rc})")
        raw = self.lib.image_size(pi)
        return [out[i * bound:i * bound + raw].copy() for i in range(n)], pi

    def decode_batch_crop_resize_tensor(self, streams, rects, out_width, out_height, dtype, layout, scale, bias, mirror=None, out=None, out_stride=None,
                                        device_in=None, in_stride=None, sizes=None):
        """gpujpeg_amd_decoder_decode_batch_crop_resize_tensor: decode_batch_crop_resize whose frames come as normalised float tensors -- element
        (c, j, i) = byte * scale[c] + bias[c] in dtype (TENSOR_F32 / _F16 / _BF16), laid out as layout says (TENSOR_CHW / _HWC); the definition:
        include/gpujpeg_amd_ext.h. The usual recipe: scale = 1 / (255 std), bias = -mean / std. streams / device_in, in_stride, sizes, rects and mirror as
        for decode_batch_crop_resize. out: an integer pointer (device or host memory) with out_stride = bytes between two frames, or an object with
        data_ptr(), element_size() and is_contiguous() -- a torch tensor on the GPU or the CPU, contiguous, of the dtype's element size and with room for
        the frames; its first dimension is the frame. Returns (None, ImageParameters) then. Without out the frames come back as one numpy array of shape
        (n, C, OH, OW) or (n, OH, OW, C), float32, float16, or uint16 holding the bit patterns of bfloat16."""
        if not hasattr(self.lib.L, "gpujpeg_amd_decoder_decode_batch_crop_resize_tensor"):
            raise RuntimeError("this library has no gpujpeg_amd_decoder_decode_batch_crop_resize_tensor")
        if device_in is None:
            sizes = [int(x.size) for x in streams]
            in_stride = (max(sizes) + 64 + 15) & ~15
            buf = np.zeros(in_stride * len(sizes), np.uint8)
            for i, x in enumerate(streams):
                buf[i * in_stride:i * in_stride + x.size] = x
            self._keep = buf
            base = buf.ctypes.data
        else:
            base = int(device_in)
        n = len(sizes)
        if len(rects) != n or (mirror is not None and len(mirror) != n):
            raise ValueError("decode_batch_crop_resize_tensor needs one rectangle (and, with mirror, one flag) per stream")
        fmt = tensor_format(dtype, layout, scale, bias)
        if fmt.dtype not in TENSOR_ELSIZE:
            raise ValueError(f"decode_batch_crop_resize_tensor: unknown dtype {dtype}")
        elsize = TENSOR_ELSIZE[fmt.dtype]
        csz = (C.c_size_t * n)(*sizes)
        rc4 = (C.c_int * (4 * n))(*[int(v) for r in rects for v in r])
        mir = None if mirror is None else (C.c_uint8 * n)(*[1 if m else 0 for m in mirror])
        pi = ImageParameters()
        call = self.lib.L.gpujpeg_amd_decoder_decode_batch_crop_resize_tensor
        if out is not None:
            if hasattr(out, "data_ptr"):  # (a torch tensor, without importing torch: frames along its first dimension)
                if not out.is_contiguous():
                    raise ValueError("decode_batch_crop_resize_tensor: out must be contiguous")
                if out.element_size() != elsize:
                    raise ValueError(f"decode_batch_crop_resize_tensor: out has elements of {out.element_size()} B, the dtype asks for {elsize} B")
                if out.shape[0] != n:
                    raise ValueError(f"decode_batch_crop_resize_tensor: out holds {out.shape[0]} frames, the call has {n}")
                ptr, out_stride = int(out.data_ptr()), int(out.numel() // n) * elsize
            else:
                if out_stride is None:
                    raise ValueError("decode_batch_crop_resize_tensor: an integer out needs out_stride")
                ptr = int(out)
            rc = call(self.h, base, in_stride, csz, n, rc4, mir, int(out_width), int(out_height), C.byref(fmt), ptr, int(out_stride), C.byref(pi))
            if rc != 0:
                raise RuntimeError(f"gpujpeg_amd_decoder_decode_batch_crop_resize_tensor failed ({rc})")
            return None, pi
        ow, oh = min(max(int(out_width), 1), 16384), min(max(int(out_height), 1), 16384)
        bound = ow * oh * 3 * elsize  # (room for three channels; a single-channel result uses a third of every slot)
        host = np.empty(bound * n, np.uint8)
        rc = call(self.h, base, in_stride, csz, n, rc4, mir, int(out_width), int(out_height), C.byref(fmt), host.ctypes.data, bound, C.byref(pi))
        if rc != 0:
            raise RuntimeError(f"gpujpeg_amd_decoder_decode_batch_crop_resize_tensor failed ({rc})")
        ch = 1 if pi.pixel_format == 0 else 3
        frames = host.reshape(n, bound)[:, :ch * ow * oh * elsize].copy().view(TENSOR_NUMPY[fmt.dtype])
        return frames.reshape((n, ch, oh, ow) if fmt.layout == TENSOR_CHW else (n, oh, ow, ch)), pi

    def prescales(self):
        """gpujpeg_amd_decoder_get_prescales: the scale s_f (1, 2, 4, 8) every frame of the last decode_batch_crop_resize call took ahead of its resample
        (set_option("dec_opt_resize_prescale", "1/8") allows up to 8; 4:2:0 streams take one only with set_option("dec_opt_resize_prescale_subsampled",
        "on")); [] when there was no such call or it failed"""
        cap = 65536
        a = (C.c_uint8 * cap)()
        n = self.lib.L.gpujpeg_amd_decoder_get_prescales(self.h, a, cap)
        return [int(a[i]) for i in range(n)]

    def region_stats(self):
        """gpujpeg_amd_decoder_get_region_stats of the last decode call: (mode 0 none / 1 selected segments / 2 every segment, restart segments
        entropy-decoded, 8x8 blocks transformed, segments in the stream)"""
        a = (C.c_long * 4)()
        self.lib.L.gpujpeg_amd_decoder_get_region_stats.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        assert self.lib.L.gpujpeg_amd_decoder_get_region_stats(self.h, a) == 0
        return tuple(int(x) for x in a)

    def progressive_stats(self):
        """gpujpeg_amd_decoder_get_progressive_stats: (rc, 1 if the last decode call's frame was progressive, scans decoded, dependency levels = entropy
        launches, scan segments = waves launched); rc -1 and zeros before the first call"""
        a = (C.c_long * 4)()
        self.lib.L.gpujpeg_amd_decoder_get_progressive_stats.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        rc = self.lib.L.gpujpeg_amd_decoder_get_progressive_stats(self.h, a)
        return (int(rc),) + tuple(int(x) for x in a)

    def progressive_batch_stats(self):
        """gpujpeg_amd_decoder_get_progressive_batch_stats: (rc, frames the batched progressive launches took, groups, entropy launches, records = waves)
        of the last batch call made with DEC_OPT_PROGRESSIVE and DEC_OPT_BATCH_PROGRESSIVE both on; (-1, 0, 0, 0, 0) after any other call"""
        a = (C.c_long * 4)()
        self.lib.L.gpujpeg_amd_decoder_get_progressive_batch_stats.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        rc = self.lib.L.gpujpeg_amd_decoder_get_progressive_batch_stats(self.h, a)
        return (int(rc),) + tuple(int(x) for x in a)

    def batch_header_stats(self):
        """gpujpeg_amd_decoder_get_batch_header_stats: (rc, frames the host admitted to the family, distinct table sets uploaded, header bytes brought to
        the host, frames whose header was fetched on its own) of the last crop-and-resize call made with DEC_OPT_BATCH_SIZES = mixed and
        DEC_OPT_BATCH_HEADERS = any; (-1, 0, 0, 0, 0) after any other call"""
        a = (C.c_long * 4)()
        self.lib.L.gpujpeg_amd_decoder_get_batch_header_stats.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        rc = self.lib.L.gpujpeg_amd_decoder_get_batch_header_stats(self.h, a)
        return (int(rc),) + tuple(int(x) for x in a)

    def batch_header_times(self):
        """gpujpeg_amd_decoder_get_batch_header_times: (rc, ms bringing device-resident headers to the host, ms parsing, ms family rule + table sets +
        geometries) of the last call batch_header_stats() describes; (-1, 0.0, 0.0, 0.0) after any other call"""
        a = (C.c_double * 3)()
        self.lib.L.gpujpeg_amd_decoder_get_batch_header_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        rc = self.lib.L.gpujpeg_amd_decoder_get_batch_header_times(self.h, a)
        return (int(rc),) + tuple(float(x) for x in a)

    def entropy_bytes(self):
        """gpujpeg_amd_decoder_get_entropy_bytes: (rc, bytes handed to the entropy decoders by the batched launches, bytes of them that were read) of the
        last batch call made with set_option(DEC_OPT_BATCH_RESTARTLESS, BATCH_RESTARTLESS_ON); (-1, 0, 0) after any other call"""
        a = (C.c_uint64 * 2)()
        self.lib.L.gpujpeg_amd_decoder_get_entropy_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        rc = self.lib.L.gpujpeg_amd_decoder_get_entropy_bytes(self.h, a)
        return int(rc), int(a[0]), int(a[1])

    def path_counters(self):
        """(speculative launches, of those without the k_marker_table launch, decoded again the careful way) of this decoder so far"""
        a = (C.c_long * 3)()
        self.lib.L.gpujpeg_amd_decoder_get_path_counters.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        assert self.lib.L.gpujpeg_amd_decoder_get_path_counters(self.h, a) == 0
        return tuple(int(x) for x in a)

    def stats(self):
        s = DurationStats()
        self.lib.L.gpujpeg_decoder_get_stats(self.h, C.byref(s))
        return s

    def set_fused(self, enabled):
        self.lib.L.gpujpeg_amd_decoder_set_fused(self.h, int(enabled))

    def keep_coefficients(self, enabled=True):
        """Leave the quantised coefficients of the following decode calls in HBM (for coefficients())."""
        self.lib.L.gpujpeg_amd_decoder_keep_coefficients(self.h, int(enabled))

    def kernel_times(self):
        ms = (C.c_float * 8)()
        if self.lib.L.gpujpeg_amd_decoder_get_kernel_times(self.h, ms) != 0:
            return None
        return list(ms)[:4]

    def idct_path(self):
        """IDCT side of the last perf_stats call: 0 full size, 1 reduced size from the coefficient planes, 2 reduced size from tokens,
        3 region from the coefficient planes, 4 region from tokens, 5 region resampled from the cover planes (crop-and-resize), 6 the same with a frame
        reduced ahead of the resample (dec_opt_resize_prescale), 7 region resampled with the antialiased filter (dec_opt_resize_filter=antialias),
        8 as 6 with a frame of a 4:2:0 stream reduced per component (dec_opt_resize_prescale_subsampled=on)"""
        ms = (C.c_float * 8)()
        if self.lib.L.gpujpeg_amd_decoder_get_kernel_times(self.h, ms) != 0:
            return None
        return int(ms[4])

    def coefficients(self, count):
        a = np.empty(count, np.int16)
        n = self.lib.L.gpujpeg_amd_decoder_read_coefficients(self.h, a.ctypes.data_as(C.POINTER(C.c_int16)), count)
        return a[:n]

    def planes(self, count):
        a = np.empty(count, np.uint8)
        n = self.lib.L.gpujpeg_amd_decoder_read_planes(self.h, a.ctypes.data_as(C.POINTER(C.c_uint8)), count)
        return a[:n]

    def close(self):
        if self.h:
            self.lib.L.gpujpeg_decoder_destroy(self.h)
            self.h = None

    __del__ = close
