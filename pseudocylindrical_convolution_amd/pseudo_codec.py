"""360-degree image codec driver (reference: pseudo_codec.py:27-356).

Inference-time entropy model (EntEncoder / EntDecoder wavefront loops), the
end-to-end PseudoEncoder / PseudoDecoder, evaluation and the command line.
Differences from the reference, all additive:
  * any ERP size with height % 256 == 0 and width % 16 == 0 (the reference
    hard-codes 512x1024 latents, pseudo_codec.py:206,209,229-234); the defaults
    reproduce the reference exactly;
  * any other ERP size h x w through the pole / seam padding rule of erp_size.py:
    coded at coded_size(h, w), the decoder crops back (container version 2,
    command line --native-size);
  * --test --ws adds WS-PSNR / WS-SSIM (sphere_metrics.py) beside the viewport figures, --ms-ssim with it WS-MS-SSIM;
  * --test --sphere / --rd --sphere add S-PSNR-NN / S-PSNR-I / CPP-PSNR (sphere_points.py: both pictures sampled at the
    same points of the sphere) and, for a file coded with --code-size, the same three of the reconstruction at the coded
    size against the source at its own;
  * --test / --rd --projection --cube-metrics add CUBE-WS-PSNR and CUBE-S-PSNR-NN / -I / CUBE-CPP-PSNR: the cube picture
    against the reconstructed cube picture, both read as cube pictures (cube.py, weighted_metrics.py); --cube-ssim adds
    CUBE-WS-SSIM of the same pair (cube.ws_ssim: every face continued from its neighbours by the window's radius);
  * --yuv / --yuv-out code raw YUV 4:2:0 files (yuv.py: yuv420p, nv12, yuv420p10le), one code file per frame, the
    colour conversion on the GPU; --test --ws then adds WS-PSNR-Y/U/V.  The stream and the container are the RGB ones:
    the decoder is told the pixel format on the command line;
  * --rd scores images without writing a file: the rate from the CDF rows (rate.py), the distortion from the
    reconstruction of the encoder's own symbols -- no arithmetic coder, no entropy decoder;
  * images are read/written with PIL (cv2 is not required) in the reference's BGR
    channel order, so its checkpoints stay valid.
Module / parameter names are the reference's, so `{idx}_encoder.pt`,
`{idx}_decoder.pt` and `{idx}_ent.pt` load with strict=True (pseudo_codec.py:223-227).
"""
import argparse
import math
import os
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from .PCONV_operator import (DExtract2, DExtract2Batch, DInput2, Dtow, EntropyAdd, EntropyBatchGmmTable,
                             EntropyContextNew, EntropyConv2Batch, EntropyCtxPadRun2, Extract, MultiProject,
                             PseudoContextV2, PseudoDQUANT, PseudoFillV2, PseudoQUANTV2, SphereSlice,
                             SphereUslice, SSIM, backend)
from .model_zoo_v2 import ClipData, DecoderV2, EncoderV2
from . import container
from .erp_size import coded_size  # noqa: F401  (re-exported beside latent_shape)
from . import sphere_metrics
from . import yuv
from .frame_geometry import FrameGeometry

psnr_f = lambda xa: 10 * math.log10(1. / xa)

model_ssim_list = ['1_56', '2_56', '3_56', '4_56', '5_112', '6_112', '7_112', '8_192', '9_192']
ssim_channel_list = [56, 56, 56, 56, 112, 112, 112, 192, 192]
model_mse_list = ['1_56', '2_56', '3_56', '4_112', '5_112', '6_112', '7_112', '8_192', '9_192', '10_192']
mse_channel_list = [56, 56, 56, 112, 112, 112, 112, 192, 192, 192]
mse_model_dir = './demo/mse'
ssim_model_dir = './demo/ssim'

NPART = 16          # latitude tiles (pseudo_codec.py:166)
CHANNELS = 192      # transform width and code channels
QUANT_LEVELS = 8
DOWN = 16           # spatial down-sampling of the analysis transform


def latent_shape(height, width, npart=NPART):
    """(rows per tile, columns) of the code tensor for an ERP of height x width."""
    if height % (npart * DOWN) or width % DOWN:
        raise ValueError('ERP size %dx%d: height must be a multiple of %d and width of %d'
                         % (height, width, npart * DOWN, DOWN))
    return height // npart // DOWN, width // DOWN


class EntropyConvDBT(nn.Module):
    """causal halo update + masked conv with three weight sets (reference: pseudo_codec.py:27-38)."""

    def __init__(self, batch, ngroups, cin, cout, hidden, npart, out_layer, ctx, device_id, act=True):
        super(EntropyConvDBT, self).__init__()
        self.pad = EntropyCtxPadRun2(2, npart, ngroups, ctx, not hidden, device=device_id)
        self.conv = EntropyConv2Batch(npart, ngroups, cin, cout, 5, ctx, 2, 0 if out_layer else 2, batch=batch,
                                      hidden=hidden, act=act, device=device_id)

    def forward(self, x):
        return self.conv(self.pad(x))


class EntropyResidualBlockDBT(nn.Module):
    """(reference: pseudo_codec.py:40-51)"""

    def __init__(self, batch, ngroups, cpn, npart, ctx, device_id=0):
        super(EntropyResidualBlockDBT, self).__init__()
        self.conv1 = EntropyConvDBT(batch, ngroups, cpn, cpn, True, npart, False, ctx, device_id, True)
        self.conv2 = EntropyConvDBT(batch, ngroups, cpn, cpn, True, npart, False, ctx, device_id, True)
        self.add = EntropyAdd(npart, cpn * ngroups, ngroups, 2, ctx, device=device_id)

    def forward(self, x):
        return self.add(self.conv2(self.conv1(x)), x)


_STEPPED = (EntropyConv2Batch, EntropyCtxPadRun2, EntropyAdd, DInput2, DExtract2, DExtract2Batch)


@torch.no_grad()
def restart_entropy_network(m):
    """reset the step counter of every wavefront op (reference: pseudo_codec.py:53-66)"""
    if isinstance(m, _STEPPED):
        m.restart()


class _EntropyModel(nn.Module):
    """what the encoder and decoder sides share: context, input scatter, the
    12-layer three-headed masked network, GMM table"""

    def __init__(self, ngroup, npart, opt_f, bin_num, gid):
        super(_EntropyModel, self).__init__()
        self.cuda = backend.device_of(gid)
        self.ctx2 = EntropyContextNew(npart, opt=opt_f, device=gid)
        self.ipt = DInput2(ngroup, npart, self.ctx2, 2, -3.5, 3, device=gid)
        self.npart, self.ngroup = npart, ngroup
        self.fill = PseudoFillV2(0, npart, self.ctx2, 0, device=gid)
        self.mcoder = None
        self.bias = (bin_num - 1) / 2.
        layers = [EntropyConvDBT(3, ngroup, 1, 3, False, npart, False, self.ctx2, gid, True)]
        layers += [EntropyResidualBlockDBT(3, ngroup, 3, npart, self.ctx2, gid) for _ in range(5)]
        layers += [EntropyConvDBT(3, ngroup, 3, 3, True, npart, True, self.ctx2, gid, False)]
        self.net = nn.Sequential(*layers)
        self.ext = DExtract2Batch(npart, ngroup, self.ctx2, device=gid)
        self.gmm = EntropyBatchGmmTable(bin_num, self.bias, 3, 65536, device=gid)
        backend.watch_state_dict(self)  # reloaded weights drop the engine's repacked slabs

    def start(self, code_name='./tmp/data'):
        self.apply(restart_entropy_network)
        self.mcoder = backend.coder().coder(code_name)

    def steps(self, h_full, w):
        return h_full + w + self.ngroup - 2

    def tables(self, packed):
        """one wavefront step: scatter `packed` symbols of the previous step, run
        the network, return (integer CDF rows on the CPU, number of rows)"""
        b = self.ipt(packed)
        z, le = self.ext(self.net(b))
        vec = self.gmm(z, le)
        return b, vec.type(torch.int32).to('cpu'), int(le[0].item())


class EntEncoder(_EntropyModel):
    """(reference: pseudo_codec.py:68-114)"""

    def __init__(self, ngroup, npart=16, opt_f=True, bin_num=8, gid=0):
        super(EntEncoder, self).__init__(ngroup, npart, opt_f, bin_num, gid)
        self.ext_label = DExtract2(npart, ngroup, True, self.ctx2, device=gid)
        self.net = self.net.to(self.cuda)

    def forward(self, data):
        with torch.no_grad():
            data = self.fill(data)
            h, w = data.shape[2:]
            self.ctx2.setup_context(w)
            self.mcoder.start_encoder()
            h_full = h * self.npart
            label = torch.zeros((1, 1, h_full, w), dtype=torch.float32).to(self.cuda)
            for _ in range(self.steps(h_full, w)):
                _, pred, ln = self.tables(label)
                label, _ = self.ext_label(data)
                self.mcoder.encodes(pred, 8, label.type(torch.int32).to('cpu'), ln)
            self.mcoder.end_encoder()


class EntDecoder(_EntropyModel):
    """(reference: pseudo_codec.py:117-160)"""

    def __init__(self, ngroup, npart=16, opt_f=True, bin_num=8, gid=0):
        super(EntDecoder, self).__init__(ngroup, npart, opt_f, bin_num, gid)
        self.net = self.net.to(self.cuda)

    def forward(self, h, w):
        with torch.no_grad():
            self.ctx2.setup_context(w)
            self.mcoder.start_decoder()
            h_full = h * self.npart
            pout = torch.zeros((1, 1, h_full, w), dtype=torch.float32).to(self.cuda)
            b = None
            for _ in range(self.steps(h_full, w)):
                b, pred, ln = self.tables(pout)
                pout = self.mcoder.decodes(pred.view(-1, 9), 8, ln).to(self.cuda).view(1, 1, h_full, w).contiguous()
            code = (b[:self.npart, :, 2:-2, 2:-2] + self.bias).contiguous()
            return self.fill(code)


class PseudoEncoder(nn.Module):
    """ERP image -> code file (reference: pseudo_codec.py:162-186)"""

    def __init__(self, valid_dim, device_id):
        super(PseudoEncoder, self).__init__()
        npart, opt = NPART, True
        dev = backend.device_of(device_id)
        self.slice = SphereSlice(npart, pad=0, opt=opt, device=device_id)
        self.ctx = PseudoContextV2(npart, opt, device=device_id)
        self.encoder = EncoderV2(CHANNELS, CHANNELS, npart, self.ctx, device_id).to(dev)
        self.quant = PseudoQUANTV2(CHANNELS, QUANT_LEVELS, npart, self.ctx, device_id=device_id, ntop=2)
        self.valid_dim = valid_dim
        self.ext = Extract(valid_dim)
        self.mean_val = (QUANT_LEVELS - 1) / 2.
        self.dtw = Dtow(2, True, device_id)
        self.ent = EntEncoder(valid_dim // 4, npart, opt, QUANT_LEVELS, gid=device_id)
        backend.watch_state_dict(self)

    def symbols(self, x):
        """quantiser indices in wavefront layout (npart, valid_dim/4, 2h, 2w)"""
        with torch.no_grad():
            _, code_i = self.quant(self.encoder(self.slice(x)))
            return self.dtw(self.ext(code_i))

    def forward(self, x, code_name, header=None, geometry=None):
        """x -> code file.  On the GPU the entropy stage runs on the native engine
        (engine.EntropyEngine: one launch per layer over all wavefront steps); the file is
        byte for byte what the op-by-op loop of `forward_per_op` writes
        (tests/test_gpu_engine.py).  PCONV_ENTROPY=per-op forces the loop.
        header: dict(model_idx=, ssim=) -> the file gets the container header (container.py) in front of
        the same payload; None = the reference's raw stream.
        geometry: the FrameGeometry x is the coded frame of (frame_geometry.py) -- x was padded from, or rotated,
        resized and padded from, another picture (a cube picture among them), which the header then records (container
        version 2 to 5) and the decoder returns to; None = x is the picture itself."""
        with torch.no_grad():
            if header is None and geometry is not None and geometry.rotated:
                raise ValueError("a headerless stream cannot carry the rotation: give a header")
            if header is None and geometry is not None and geometry.projected:
                raise ValueError("a headerless stream cannot carry the projection: give a header")
            if header is not None:
                if geometry is None:
                    geometry = FrameGeometry(x.shape[2:])
                if geometry.coded != tuple(x.shape[2:]):
                    raise ValueError("frame %s is not the coded size of %dx%d"
                                     % (tuple(x.shape[2:]), geometry.content[1], geometry.content[0]))
            hcode_i = self.symbols(x)
            eng = _native_engine(self, "enc", hcode_i)
            if eng is None:   # the coder module writes the file itself: a header goes in front of what it wrote
                self.ent.start(code_name)
                self.ent(hcode_i)
                if header is None:
                    return
                with open(code_name, "rb") as f:
                    payload = f.read()
            else:
                payload = eng.encode(self.ent.fill(hcode_i).contiguous())[0]
            if header is None:
                with open(code_name, "wb") as f:
                    f.write(payload)
            else:
                container.write_any(code_name, payload, model_idx=header["model_idx"], ssim=header["ssim"],
                                    valid_dim=self.valid_dim, **geometry.header_fields())

    def forward_per_op(self, x, code_name):
        """the reference's loop (pseudo_codec.py:97-114): ~36 op calls per wavefront step"""
        with torch.no_grad():
            hcode_i = self.symbols(x)
            self.ent.start(code_name)
            self.ent(hcode_i)


class PseudoDecoder(nn.Module):
    """code file -> ERP image (reference: pseudo_codec.py:188-213).  height/width
    default to the reference's only size."""

    def __init__(self, valid_dim, device_id):
        super(PseudoDecoder, self).__init__()
        self.npart, opt, self.channels, self.code_channels = NPART, True, CHANNELS, CHANNELS
        dev = backend.device_of(device_id)
        self.valid_dim = valid_dim
        self.uslice = SphereUslice(self.npart, pad=0, opt=opt, device=device_id)
        self.ctx = PseudoContextV2(self.npart, opt, device=device_id)
        self.decoder = DecoderV2(self.channels, self.code_channels, self.npart, self.ctx, device_id).to(dev)
        self.clip = ClipData()
        self.quant = PseudoDQUANT(self.code_channels, QUANT_LEVELS, self.npart, self.ctx, device_id=device_id)
        self.wtd = Dtow(2, False, device_id)
        self.ent = EntDecoder(self.valid_dim // 4, self.npart, opt, QUANT_LEVELS, gid=device_id)
        backend.watch_state_dict(self)

    def reconstruct(self, hcode_i):
        """symbols in wavefront layout -> image"""
        with torch.no_grad():
            code_ext = self.quant(self.wtd(hcode_i))
            code_f = torch.zeros((code_ext.shape[0], self.code_channels) + tuple(code_ext.shape[2:])).type_as(code_ext)
            code_f[:, :self.valid_dim] = code_ext
            return self.clip(self.uslice(self.decoder(code_f.contiguous())))

    def forward(self, code_name, height=512, width=1024, raw=None):
        """code file -> image; the entropy stage on the native engine when on the GPU
        (see PseudoEncoder.forward).  raw=True: the reference's headerless stream, size from the
        arguments; raw=False: the file carries the container header (container.py) and height /
        width are read from it; raw=None (default): a file that starts with a valid container
        header is read as one, anything else as a raw stream.  A size the codec does not take as it is
        (container version 2) is decoded at its coded size and cropped to the original size (erp_size.py).
        A container that records a source size (version 3) is decoded the same way and then
        resized to the source size, clamped to [0, 1] (erp_resample.py); one that records a rotation (version 4) is
        then turned back to the source's orientation (erp_rotate.py); one that records a projection (version 5) is last
        of all converted to the cube picture (cube.py)."""
        rec, geometry = self.decode_coded(code_name, height, width, raw)
        return geometry.from_coded(rec)

    def decode_coded(self, code_name, height=512, width=1024, raw=None):
        """(reconstruction at the coded size, FrameGeometry) of a code file, raw as in forward(): the geometry is the
        header's for a container, FrameGeometry.for_raw(height, width) for a headerless stream;
        geometry.from_coded(reconstruction) is the picture"""
        payload = None
        if raw is None:
            raw = container.sniff(code_name) is None
        if raw:
            if height is None or width is None:
                raise ValueError("%s has no container header: its frame size must be given (--size WxH)" % code_name)
            geometry = FrameGeometry.for_raw(height, width)
        else:
            head, payload = container.read(code_name)
            if head["valid_dim"] != self.valid_dim:
                raise container.ContainerError("file was coded with valid_dim %d, this decoder has %d"
                                               % (head["valid_dim"], self.valid_dim))
            geometry = FrameGeometry.from_header(head)
        return self._decode(code_name, geometry.coded[0], geometry.coded[1], raw, payload), geometry

    def _decode(self, code_name, height, width, raw, payload):
        with torch.no_grad():
            h, w = latent_shape(height, width, self.npart)
            eng = _native_engine(self, "dec", None, 2 * h, 2 * w)
            if eng is None:
                if not raw:   # the coder modules read files: hand them the bare payload
                    code_name = code_name + ".payload"
                    with open(code_name, "wb") as f:
                        f.write(payload)
                self.ent.start(code_name)
                try:
                    return self.reconstruct(self.ent(2 * h, 2 * w))
                finally:
                    if not raw:
                        self.ent.mcoder = None
                        os.remove(code_name)
            if raw:
                with open(code_name, "rb") as f:
                    payload = f.read()
            return self.reconstruct(eng.decode([payload]))

    def forward_per_op(self, code_name, height=512, width=1024):
        """the reference's loop (pseudo_codec.py:145-160)"""
        with torch.no_grad():
            h, w = latent_shape(height, width, self.npart)
            self.ent.start(code_name)
            return self.reconstruct(self.ent(2 * h, 2 * w))


def _native_engine(codec, which, symbols=None, h2=None, w2=None):
    """single-frame EntropyEngine bound to codec.ent, cached on the codec per latent size;
    None when the active backend has no native engine (the CPU oracle used by the tests)
    or PCONV_ENTROPY=per-op asks for the op-by-op loops"""
    import os
    ops = backend.ops()
    if os.environ.get("PCONV_ENTROPY", "native") == "per-op" or not getattr(ops, "FUSED_EPILOGUE", False):
        return None
    if symbols is not None:
        if not symbols.is_cuda:
            return None
        h2, w2 = symbols.shape[2], symbols.shape[3]
    from .engine import EntropyEngine
    cache = codec.__dict__.setdefault("_pconv_engines", {})
    key = (which, int(h2), int(w2))
    if key not in cache:
        dev = next(codec.ent.parameters()).device
        if dev.type != "cuda":
            return None
        cache[key] = EntropyEngine(codec.ent, h2, w2, 1, dev)
    else:
        cache[key].bind(codec.ent)  # parameters may have been reloaded
    return cache[key]


# -- image / checkpoint I/O ---------------------------------------------------
def read_image(path):
    """uint8 HxWx3 in BGR order (what cv2.imread returns in the reference)"""
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))[:, :, ::-1].copy()


def write_image(path, img_bgr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img_bgr[:, :, ::-1])).save(path)


def img2tensor(img, device):
    ts = torch.from_numpy(img.transpose(2, 0, 1).astype(np.float32)) / 255.
    return torch.unsqueeze(ts, 0).to(device).contiguous()


def tensor2img(data):
    return (data[0] * 255.).to('cpu').detach().numpy().transpose(1, 2, 0).astype(np.uint8)


def check_img(img, height=512, width=1024):
    """bicubic resize to the coding size when the input differs (reference: pseudo_codec.py:229-234)"""
    if img.shape[0] == height and img.shape[1] == width:
        return img
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((width, height), Image.BICUBIC))


def load_models(model, p1, p2, device):
    merged = OrderedDict(**torch.load(p1, map_location=device), **torch.load(p2, map_location=device))
    model.load_state_dict(merged)


def _load(kind, model_idx, mse, device_id):
    """(PseudoEncoder for kind "encoder" or PseudoDecoder for "decoder" of a model of the VMSE / VSSIM list, on its
    device and with its checkpoint loaded; that device)"""
    prex = model_mse_list[model_idx] if mse else model_ssim_list[model_idx]
    vd = mse_channel_list[model_idx] if mse else ssim_channel_list[model_idx]
    model_dir = mse_model_dir if mse else ssim_model_dir
    dev = backend.device_of(device_id)
    model = {"encoder": PseudoEncoder, "decoder": PseudoDecoder}[kind](vd, device_id=device_id).to(dev)
    load_models(model, '{}/{}_{}.pt'.format(model_dir, prex, kind), '{}/{}_ent.pt'.format(model_dir, prex), dev)
    return model, dev


def bitrate(path, height=512, width=1024):
    """bits per pixel of the coded payload (a container header is not counted, so the figure is
    the reference's `os.path.getsize(fc)*8/1024./512.` for the same stream, pseudo_codec.py:247,283)"""
    nbytes = os.path.getsize(path) - container.header_bytes(path)
    return nbytes * 8 / float(width) / float(height)


def img2tensor_on_device(img, device):
    """img2tensor with the division on `device`: the uint8 pixels cross the bus.  NOT the same bits on a GPU, where
    torch divides by a scalar as a multiplication by float32(1 / 255.) (126 of the 256 values are one ulp off the
    host's quotient); --code-size has coded this tensor since its first file, so it keeps it"""
    return (torch.from_numpy(np.ascontiguousarray(img)).to(device).permute(2, 0, 1).float() / 255.)[None].contiguous()


def encoding(img_list, out_list, model_idx=0, mse=True, device_id=0, height=512, width=1024, boxed=False,
             native=False, code_size=None, rotation=None, projection=None):
    """reference: pseudo_codec.py:236-247.  The files are the reference's headerless streams unless
    boxed=True (--container): then the 16-byte header of container.py goes in front of the same
    payload and the file decodes without any size / model argument.  native=True (--native-size,
    needs boxed): every image is coded at its own size, padded by the pole / seam rule of erp_size.py
    instead of resized; height / width are ignored.  code_size=(H2, W2) (--code-size, needs boxed, excludes native):
    every image is resized on the device to H2 x W2 by the sphere-aware rule of erp_resample.py (any size of at
    least 2 x 2, padded by the pole / seam rule where it is not codable); the file records both sizes (container
    version 3) and the bitrate counts the source's pixels.  rotation (--rotate, needs boxed): the triple of
    erp_rotate.units; every image is first turned into that orientation on the device (erp_rotate.py) and the file
    records it (container version 4).  projection (--projection, needs boxed): a cube.Spec; every image is a cube
    picture in its layout, taken at its own size (height / width are ignored), converted on the device to the ERP frame
    of cube.erp_size(face size) (cube.py) before everything else; the file records kind, layout and face size
    (container version 5) and the bitrate counts the cube picture's pixels."""
    if projection is not None and not boxed:
        raise ValueError("--projection needs --container: a headerless file cannot carry the projection")
    if projection is not None and native:
        raise ValueError("--projection excludes --native-size: a cube picture is always taken at its own size")
    if rotation is not None and not boxed:
        raise ValueError("--rotate needs --container: a headerless file cannot carry the rotation")
    if native and not boxed:
        raise ValueError("--native-size needs --container: a headerless file cannot carry the image size")
    if code_size is not None and (native or not boxed):
        raise ValueError("--code-size needs --container and excludes --native-size")
    t1, dev = _load("encoder", model_idx, mse, device_id)
    header = {"model_idx": model_idx, "ssim": not mse} if boxed else None
    for fn, fo in zip(img_list, out_list):
        img = read_image(fn)
        if not native and code_size is None and projection is None:
            img = check_img(img, height, width)
        geometry = FrameGeometry.for_picture(img.shape[:2], code_size, rotation, projection)
        data = img2tensor(img, dev) if code_size is None else img2tensor_on_device(img, dev)
        t1(geometry.to_coded(data), fo, header, geometry)
        print('Encoding {}, bitrate: {:.3f}bpp'.format(fn, bitrate(fo, *geometry.picture)))


def _decoder_for(code_list, model_idx, mse, device_id, raw):
    """decoder with its checkpoint loaded.  When the FIRST file carries a container header the
    model is the one it names (all container files of a call must agree); raw=True never looks"""
    head = None if raw else container.sniff(code_list[0])
    if head is not None:
        model_idx, mse = head["model_idx"], not head["ssim"]
    return _load("decoder", model_idx, mse, device_id) + (model_idx, mse)


def _decode_file(t1, fc, model_idx, mse, height, width, raw, to_source=True):
    """(reconstruction at the coded size, FrameGeometry) of one code file of a list: the sizes from its container
    header when it has one (which must name the model the decoder was built for), else from the arguments.
    to_source=False refuses a file whose picture has to be resized, rotated or converted back (version 3, 4, 5)"""
    head = None if raw else container.sniff(fc)
    if head is not None:
        if head["model_idx"] != model_idx or head["ssim"] == mse:
            raise container.ContainerError("%s was coded with another model than the first file of the list" % fc)
        if "source_height" in head and not to_source:
            raise container.ContainerError("%s was coded at a reduced size (--code-size): decode it to images" % fc)
        if "rotation" in head and not to_source:
            raise container.ContainerError("%s was coded in a rotated orientation (--rotate): decode it to images" % fc)
        if "projection" in head and not to_source:
            raise container.ContainerError("%s holds a cube picture (--projection): decode it to images" % fc)
    return t1.decode_coded(fc, height, width, raw=head is None)


def decoding(code_list, decoded_img_list, model_idx=0, mse=True, device_id=0, height=512, width=1024, raw=False,
             view=None, view_size=None, view_list=None):
    """reference: pseudo_codec.py:249-260.  view (--view: yaw, pitch, roll, hfov in degrees) with view_size = (vh, vw)
    and view_list (--view-out, one name per code file): the rectilinear view of every decoded picture (viewport.py:
    square pixels, the supersampling of viewport.plan, clamped to [0, 1]) is written beside the panorama.  A picture
    coded with --rotate / --code-size is viewed in the source's orientation and at the source's size.  A file that holds a
    cube picture (--projection, container version 5) is written as that cube picture, layout and size from the header
    alone; its view is rendered from the ERP frame the picture was converted from"""
    t1, _, model_idx, mse = _decoder_for(code_list, model_idx, mse, device_id, raw)
    for k, (fc, fo) in enumerate(zip(code_list, decoded_img_list)):
        rec, geometry = _decode_file(t1, fc, model_idx, mse, height, width, raw)
        picture = geometry.from_coded(rec, to_source="erp")
        write_image(fo, tensor2img(geometry.from_coded(rec) if geometry.projected else picture))
        print('Decoding {}, output to {}'.format(fc, fo))
        if view is not None:
            from . import viewport
            seen = viewport.render(picture, viewport.view(*view, size=view_size), view_size, clamp=True)
            write_image(view_list[k], tensor2img(seen))
            print('Viewport {}x{} of {}, output to {}'.format(view_size[1], view_size[0], fc, view_list[k]))


class ViewportMetrics(object):
    """viewport PSNR / SSIM of the paper: 14 rectilinear views, 171x256, FoV pi/2
    (reference: pseudo_codec.py:270-282)"""

    def __init__(self, device_id=0):
        dev = backend.device_of(device_id)
        self.pr1 = MultiProject(171, int(171 * 1.5), 0.5, False, device_id).to(dev)
        self.pr2 = MultiProject(171, int(171 * 1.5), 0.5, False, device_id).to(dev)
        self.sim_func = SSIM(11, 3).to(dev)

    def __call__(self, original, decoded):
        x, y = self.pr1(original), self.pr2(decoded)
        mse_loss = torch.mean((x - y) ** 2).item()
        return psnr_f(mse_loss), self.sim_func(x, y).item()


class SphericalMetrics(object):
    """WS-PSNR / WS-SSIM of an ERP image (sphere_metrics.py): every row weighted by the area it covers on the sphere.
    Called on (original, decoded) -- uint8 (h, w, 3) images as read_image / tensor2img give them, or batches of one
    frame in either layout sphere_metrics takes -- it returns (WS-PSNR in dB, WS-SSIM), computed on the GPU by the
    HIP kernel, on the CPU by the float64 torch path (oracle backend)."""

    def __init__(self, device_id=0, weighting="ws"):
        self.dev = backend.device_of(device_id)
        self.weighting = weighting

    def _frames(self, img):
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(np.ascontiguousarray(img))[None]
        return img.to(self.dev).contiguous()

    def __call__(self, original, decoded):
        wmse, wssim = sphere_metrics.metrics(self._frames(original), self._frames(decoded), self.weighting)[0].tolist()
        return sphere_metrics.psnr(wmse), wssim

    def ms_ssim(self, original, decoded):
        """WS-MS-SSIM of the pair (--ms-ssim): five scales, images of at least 16 x 16"""
        return sphere_metrics.ws_ms_ssim(self._frames(original), self._frames(decoded), self.weighting)[0].item()


class ViewportScore(object):
    """--vp: PSNR / SSIM of the 14 paper directions rendered by viewport.py at a size that follows the picture (default
    vw = w // 4, vh = (2 vw + 1) // 3: 256x171 at 1024 columns, 1024x683 at 4096) or at size = (vh, vw), anti-aliased by
    the rule of viewport.plan.  Called on (original, decoded), float32 (1, 3, h, w) on the device, it returns (PSNR in dB
    of the views' mean MSE, the views' mean SSIM, the text that names the views).  One renderer per picture size"""

    def __init__(self, device_id=0, size=None):
        self.dev = torch.device(backend.device_of(device_id))
        self.size = size
        self.renderers = {}

    def __call__(self, original, decoded):
        from . import viewport
        h, w = original.shape[2:]
        if (h, w) not in self.renderers:
            size = self.size if self.size is not None else ((2 * (w // 4) + 1) // 3, w // 4)
            self.renderers[(h, w)] = viewport.Renderer(h, w, viewport.paper_views(size), size, device=self.dev)
        r = self.renderers[(h, w)]
        mse_loss, ssim = viewport.metrics(r, original.to(self.dev).contiguous(), decoded.to(self.dev).contiguous())[0].tolist()
        return sphere_metrics.psnr(mse_loss), ssim, '({} views {}x{}, ss={})'.format(len(r.views), r.vw, r.vh, r.ss)


class SphereScore(object):
    """--sphere: S-PSNR-NN, S-PSNR-I (the icosphere of level 8) and CPP-PSNR (the CPP grid of the original's size) of
    sphere_points.py.  Called on (original, decoded), float32 (1, 3, h, w) batches of ANY two sizes, it returns the three
    figures in dB: the HIP kernels on the GPU, the torch twins on the CPU (oracle backend)"""

    def __init__(self, device_id=0):
        self.dev = torch.device(backend.device_of(device_id))

    def __call__(self, original, decoded):
        from . import sphere_points
        x, y = original.to(self.dev).contiguous(), decoded.to(self.dev).contiguous()
        return tuple(f(x, y)[0].item() for f in (sphere_points.s_psnr_nn, sphere_points.s_psnr_i, sphere_points.cpp_psnr))


_VIEWPORT = 'Bitrate:{:.3f}bpp, PSNR:{:.2f}dB, SSIM:{:.4f}'
_WS = 'WS-PSNR:{:.2f}dB, WS-SSIM:{:.4f}'
_WS_YUV = 'WS-PSNR-Y:{:.2f}dB, WS-PSNR-U:{:.2f}dB, WS-PSNR-V:{:.2f}dB'
_WS_MS = 'WS-MS-SSIM:{:.4f}'
_VP = 'VP-PSNR:{:.2f}dB, VP-SSIM:{:.4f} '
_SPHERE = 'S-PSNR-NN:{:.2f}dB, S-PSNR-I:{:.2f}dB, CPP-PSNR:{:.2f}dB'
_SPHERE_CODED = _SPHERE + ' (coded size)'


def _vp_row(scorer, rows, texts, original, decoded):
    """--vp: the two figures join the image's row, its line is printed and its text kept for the average's line"""
    pr, ssim, text = scorer(original, decoded)
    rows[-1] += (pr, ssim)
    texts.append(text)
    print(' ' + _VP.format(pr, ssim) + text)


def _vp_line(texts):
    """the format of the average's --vp line: the images' text when they agree, else the bare figures"""
    return _VP + (texts[0] if len(set(texts)) == 1 else '(sizes differ)')


def _sphere_row(scorer, rows, coded, original, decoded, at_coded_size):
    """--sphere: the three figures of the source against the end-to-end reconstruction join the image's row and its line
    is printed; at_coded_size (the reconstruction at the coded size of a file coded with --code-size, or None) gets a
    second line, the source at its own size against that picture at its own: no resize in between"""
    rows[-1] += scorer(original, decoded)
    print(' ' + _SPHERE.format(*rows[-1][-3:]))
    coded.append(None if at_coded_size is None else scorer(original, at_coded_size))
    if coded[-1] is not None:
        print(' ' + _SPHERE_CODED.format(*coded[-1]))


def _sphere_lines(rows, coded):
    """--sphere: the formats of the average's lines; the coded-size figures join the rows (their last three columns) and
    get their line when every image has them"""
    if not coded:
        return []
    if any(c is None for c in coded):
        return [_SPHERE]
    rows[:] = [r + c for r, c in zip(rows, coded)]
    return [_SPHERE, _SPHERE_CODED]


def _report(rows, lines):
    """print the 'Average Performance' block of --test / --rd: the column averages of `rows`, each format string of
    `lines` taking the next columns it has fields for; returns rows"""
    print('-' * 53 + '\nAverage Performance\n' + '-' * 53)
    avg = list(np.average(np.array(rows), axis=0))
    for line in lines:
        n = line.count('{')
        print(line.format(*avg[:n]))
        avg = avg[n:]
    return rows


_CUBE = 'CUBE-PSNR:{:.2f}dB'
_CUBE_WS = 'CUBE-WS-PSNR:{:.2f}dB'
_CUBE_SPHERE = 'CUBE-S-PSNR-NN:{:.2f}dB, CUBE-S-PSNR-I:{:.2f}dB, CUBE-CPP-PSNR:{:.2f}dB'
_CUBE_SSIM = 'CUBE-WS-SSIM:{:.4f}'


def _cube_picture(img, geometry, name):
    """the image as the cube picture the geometry describes; a picture of another size is refused, not resized"""
    if tuple(img.shape[:2]) != geometry.picture:
        raise ValueError("%s is %dx%d, the cube picture (%s, %s, face size %d) is %dx%d"
                         % (name, img.shape[1], img.shape[0], geometry.projection.kind, geometry.projection.layout,
                            geometry.face, geometry.picture[1], geometry.picture[0]))
    return img


def _cube_sides(picture, geometry, rdata, dev):
    """(the ERP frame the codec saw of the uint8 cube picture, the float tensor the encoder converted it to; the plain
    PSNR in dB of the cube picture against the ERP reconstruction `rdata` converted back; that pair of cube pictures, for
    _cube_metrics)"""
    from . import cube
    data = img2tensor(picture, dev)
    erp = cube.to_erp(data, geometry.source, geometry.projection, clamp=True)
    back = cube.from_erp(rdata, geometry.face, geometry.projection, clamp=True)
    return erp, _plain_psnr(data, back), (data, back)


def _cube_metrics(picture, back, projection):
    """--cube-metrics: (CUBE-WS-PSNR, CUBE-S-PSNR-NN, CUBE-S-PSNR-I, CUBE-CPP-PSNR) in dB of the original cube picture
    against the reconstructed cube picture, both read as cube pictures: every pixel weighted by its solid angle, and both
    sampled at the same points of the sphere with no conversion in between (cube.ws_psnr, cube.s_psnr_nn / s_psnr_i /
    cpp_psnr); the lines are printed"""
    from . import cube
    x, y = picture.contiguous(), back.contiguous()
    figures = (cube.ws_psnr(x, y, projection)[0].item(),) + tuple(
        f(x, y, projection, projection)[0].item() for f in (cube.s_psnr_nn, cube.s_psnr_i, cube.cpp_psnr))
    print(' ' + _CUBE_WS.format(figures[0]))
    print(' ' + _CUBE_SPHERE.format(*figures[1:]))
    return figures


def _cube_ssim(picture, back, projection):
    """--cube-ssim: CUBE-WS-SSIM of the original cube picture against the reconstructed cube picture (cube.ws_ssim: the
    faces continued from their neighbours by the SSIM window's radius, every pixel weighted by its solid angle); the line
    is printed"""
    from . import cube
    figure = cube.ws_ssim(picture.contiguous(), back.contiguous(), projection)[0].item()
    print(' ' + _CUBE_SSIM.format(figure))
    return figure


def _plain_psnr(x, y):
    mse = ((x - y).double() ** 2).mean().item()
    return 10.0 * math.log10(1.0 / mse) if mse > 0 else float("inf")


def _cube_lines(rows, cubes, on_cube=(), on_ssim=()):
    """--projection: the format of the average's CUBE-PSNR line; the figures join the rows as their last column when
    every file holds a cube picture.  on_cube (--cube-metrics: _cube_metrics' four figures per image): four more columns
    and two more lines.  on_ssim (--cube-ssim: _cube_ssim's figure per image): one more column and line, the last"""
    if not cubes or any(c is None for c in cubes):
        return []
    rows[:] = [r + (c,) for r, c in zip(rows, cubes)]
    lines = [_CUBE]
    if on_cube:
        rows[:] = [r + tuple(m) for r, m in zip(rows, on_cube)]
        lines += [_CUBE_WS, _CUBE_SPHERE]
    if on_ssim:
        rows[:] = [r + (m,) for r, m in zip(rows, on_ssim)]
        lines += [_CUBE_SSIM]
    return lines


def decoding_and_test(code_list, img_list, model_idx=0, mse=True, device_id=0, height=512, width=1024, raw=False,
                      ws=False, rotation=None, ms_ssim=False, vp=None, sphere=False, projection=None, cube_metrics=False,
                      cube_ssim=False):
    """reference: pseudo_codec.py:263-290.  sphere=True (--sphere): three more columns and one more line after everything
    else, SphereScore's S-PSNR-NN / S-PSNR-I / CPP-PSNR of the source against the end-to-end reconstruction (the float
    tensors, both at the source size); a file coded at a reduced size and not rotated gets a second line, `(coded size)`,
    and when every file has it three further columns: the source at its own size against the reconstruction at the
    coded size, sampled at the same points of the sphere.  vp (--vp: True, or a size (vh, vw)): two more columns and one more line, the
    PSNR / SSIM of ViewportScore, after whatever ws adds.  ws=True (--ws): each row also carries the WS-PSNR and WS-SSIM of the
    decoded image as written (tensor2img) against the source at the image's own size: (bpp, vpsnr, vssim, ws_psnr,
    ws_ssim), with a WS line per image and for the average.  A file coded at a reduced size (--code-size, container
    version 3) is scored end to end: the picture resized back to the source size against the source, bpp over the
    source's pixels; so is a file coded in a rotated orientation (--rotate, version 4): the picture turned back against
    the unrotated source.  rotation (--test --rotate): the triple every file must record, a ContainerError otherwise.
    ms_ssim=True (--ms-ssim, with ws): one more line and a last column, the WS-MS-SSIM of the same pair.
    A file that holds a cube picture (--projection, version 5): the image is the cube picture; every line above is
    computed on the ERP frame the codec saw (the cube picture converted as the encoder converts it) against the ERP
    reconstruction, bpp over the cube picture's pixels, and one more line and a last column follow, CUBE-PSNR: the plain
    PSNR of the cube picture against the reconstruction converted back.  projection (--test --projection): the spec every
    file must record, a ContainerError otherwise.  cube_metrics (--cube-metrics, with projection): after the CUBE-PSNR
    line two more lines and four more columns, _cube_metrics' figures of the cube picture against the reconstructed cube
    picture.  cube_ssim (--cube-ssim, with projection): after all of these one more line and a last column, _cube_ssim's
    CUBE-WS-SSIM of the same pair"""
    t1, dev, model_idx, mse = _decoder_for(code_list, model_idx, mse, device_id, raw)
    metrics = ViewportMetrics(device_id)
    spherical = SphericalMetrics(device_id) if ws else None
    scorer, texts = (ViewportScore(device_id, None if vp is True else vp), []) if vp else (None, [])
    on_sphere, coded = SphereScore(device_id) if sphere else None, []
    rows, cubes, on_cube, on_ssim = [], [], [], []
    for fc, fn in zip(code_list, img_list):
        rec, geometry = _decode_file(t1, fc, model_idx, mse, height, width, raw)
        if rotation is not None and geometry.rotation != tuple(rotation):
            raise container.ContainerError("%s records the rotation %s, --rotate says %s" % (fc, geometry.rotation, tuple(rotation)))
        if projection is not None and geometry.projection != projection:
            raise container.ContainerError("%s records the projection %s, --projection says %s"
                                           % (fc, geometry.projection and tuple(geometry.projection), tuple(projection)))
        rdata = geometry.from_coded(rec, to_source="erp")
        cube_psnr = None
        if geometry.projected:
            picture = _cube_picture(read_image(fn), geometry, fn)
            data, cube_psnr, cube_pair = _cube_sides(picture, geometry, rdata, dev)
            img = tensor2img(data)
        else:
            img = check_img(read_image(fn), *geometry.source)
            data = img2tensor(img, dev)
        pr, vssim = metrics(data, rdata)
        rt = bitrate(fc, *geometry.picture)
        rows.append((rt, pr, vssim))
        print(('Decoding {}, compare it to {} \n ' + _VIEWPORT).format(fc, fn, rt, pr, vssim))
        if ws:
            rows[-1] += spherical(img, tensor2img(rdata))
            print(' ' + _WS.format(*rows[-1][3:]))
            if ms_ssim:
                rows[-1] += (spherical.ms_ssim(img, tensor2img(rdata)),)
                print(' ' + _WS_MS.format(rows[-1][-1]))
        if vp:
            _vp_row(scorer, rows, texts, data, rdata)
        if sphere:
            small = geometry.from_coded(rec, to_source=False) if geometry.resized and not geometry.rotated else None
            _sphere_row(on_sphere, rows, coded, data, rdata, small)
        cubes.append(cube_psnr)
        if cube_psnr is not None:
            print(' ' + _CUBE.format(cube_psnr))
            if cube_metrics:
                on_cube.append(_cube_metrics(*cube_pair, geometry.projection))
            if cube_ssim:
                on_ssim.append(_cube_ssim(*cube_pair, geometry.projection))
    return _report(rows, (([_VIEWPORT, _WS] + [_WS_MS] * bool(ms_ssim)) if ws else [_VIEWPORT]) + [_vp_line(texts)] * bool(vp)
                   + _sphere_lines(rows, coded) + _cube_lines(rows, cubes, on_cube, on_ssim))


def rate_distortion(img_list, model_idx=0, mse=True, device_id=0, height=512, width=1024, native=False, ws=False,
                    code_size=None, rotation=None, ms_ssim=False, vp=None, sphere=False, projection=None, cube_metrics=False,
                    cube_ssim=False):
    """--rd: what encoding() + decoding_and_test() report for the images, without a file in between.  The rate is
    the code length of the CDF rows the coder would get (rate.py: within a few bits of the stream), the
    reconstruction is the synthesis of the encoder's own symbols -- what the entropy decoder would hand back.
    Needs the native engine (GPU).  native=True (--native-size): every image at its own size, padded by the rule of
    erp_size.py; otherwise resized to height x width as --enc does.  code_size=(H2, W2) (--code-size): every image is
    coded at H2 x W2 under the rule of erp_resample.py and scored end to end at its own size, bpp over its own pixels.
    rotation (--rotate): every image is coded in that orientation (erp_rotate.py) and scored, turned back, against the
    unrotated source.
    Rows: (bpp, vpsnr, vssim[, ws_psnr, ws_ssim[, ws_ms_ssim]]): the last with ms_ssim=True (--ms-ssim); vp (--vp) adds
    ViewportScore's two columns at the end, as in decoding_and_test; sphere (--sphere) then adds SphereScore's three, and
    with code_size and no rotation the three of the coded-size line, as in decoding_and_test.
    projection (--projection): every image is a cube picture taken at its own size; the lines are computed on the ERP
    frame the codec saw, bpp over the cube picture's pixels, and CUBE-PSNR is the last line and column, as in
    decoding_and_test; cube_metrics (--cube-metrics) adds _cube_metrics' two lines and four columns after it, cube_ssim
    (--cube-ssim) _cube_ssim's line and column after those."""
    from .engine import CodecEngine
    from . import rate
    (enc, dev), (dec, _) = _load("encoder", model_idx, mse, device_id), _load("decoder", model_idx, mse, device_id)
    codec = CodecEngine(enc.valid_dim, device_id, enc, dec)
    metrics = ViewportMetrics(device_id)
    spherical = SphericalMetrics(device_id) if ws else None
    scorer, texts = (ViewportScore(device_id, None if vp is True else vp), []) if vp else (None, [])
    on_sphere, coded = SphereScore(device_id) if sphere else None, []
    rows, cubes, on_cube, on_ssim = [], [], [], []
    for fn in img_list:
        img = read_image(fn)
        if not native and code_size is None and projection is None:
            img = check_img(img, height, width)
        h, w = img.shape[:2]
        data = img2tensor(img, dev)
        picture = None
        if projection is not None:
            from . import cube
            geometry = FrameGeometry.for_picture(img.shape[:2], None, None, projection)
            picture, data = data, cube.to_erp(data, geometry.source, projection, clamp=True)
            img = tensor2img(data)
        small = None
        if sphere:
            bits, rdata, small = codec.evaluate(data, code_size=code_size, rotation=rotation, coded=True)
        else:
            bits, rdata = codec.evaluate(data, code_size=code_size, rotation=rotation)
        pr, vssim = metrics(data, rdata)
        rt = rate.bpp(bits, h, w)[0].item()
        rows.append((rt, pr, vssim))
        print('Estimating {} \n Bitrate:{:.3f}bpp (tables), PSNR:{:.2f}dB, SSIM:{:.4f}'.format(fn, rt, pr, vssim))
        if ws:
            rows[-1] += spherical(img, tensor2img(rdata))
            print(' ' + _WS.format(*rows[-1][3:]))
            if ms_ssim:
                rows[-1] += (spherical.ms_ssim(img, tensor2img(rdata)),)
                print(' ' + _WS_MS.format(rows[-1][-1]))
        if vp:
            _vp_row(scorer, rows, texts, data, rdata)
        if sphere:
            _sphere_row(on_sphere, rows, coded, data, rdata, small)
        if picture is not None:
            back = cube.from_erp(rdata, geometry.face, projection, clamp=True)
            cubes.append(_plain_psnr(picture, back))
            print(' ' + _CUBE.format(cubes[-1]))
            if cube_metrics:
                on_cube.append(_cube_metrics(picture, back, projection))
            if cube_ssim:
                on_ssim.append(_cube_ssim(picture, back, projection))
    return _report(rows, (([_VIEWPORT, _WS] + [_WS_MS] * bool(ms_ssim)) if ws else [_VIEWPORT]) + [_vp_line(texts)] * bool(vp)
                   + _sphere_lines(rows, coded) + _cube_lines(rows, cubes, on_cube, on_ssim))


def _yuv_rgb(frames, h, w, yuv_opts, dev):
    """frame buffers (n, frame_elems) -> the codec's input (n, 3, H, W) at the coded size.  yuv.to_rgb gives R, G, B
    planes; the checkpoints were trained on cv2's B, G, R order (read_image), so the planes are reversed"""
    return yuv.to_rgb(frames.to(dev), h, w, **yuv_opts).flip(1).contiguous()


def _rgb_yuv(rec, h, w, yuv_opts):
    """the decoder's reconstruction at the coded size -> frame buffers on the CPU (the inverse of _yuv_rgb)"""
    return yuv.from_rgb(rec.flip(1).contiguous(), h, w, **yuv_opts).cpu()


def encoding_yuv(path, out_list, height, width, yuv_opts, start=0, model_idx=0, mse=True, device_id=0, boxed=False):
    """--enc --yuv: frames start .. start+len(out_list)-1 of a raw .yuv file of height x width, one code file each.
    Every frame is coded at its own size (converted and padded to the coded size in one pass, yuv.to_rgb);
    boxed=True (--container) records that size, a headerless file is decoded with --size."""
    t1, dev = _load("encoder", model_idx, mse, device_id)
    header = {"model_idx": model_idx, "ssim": not mse} if boxed else None
    geometry = FrameGeometry((height, width))
    frames = yuv.read_frames(path, height, width, yuv_opts["fmt"], start, len(out_list))
    for k, fo in enumerate(out_list):
        t1(_yuv_rgb(frames[k:k + 1], height, width, yuv_opts, dev), fo, header, geometry)
        print('Encoding {} frame {}, bitrate: {:.3f}bpp'.format(path, start + k, bitrate(fo, *geometry.source)))


def decoding_yuv(code_list, path, yuv_opts, height=None, width=None, model_idx=0, mse=True, device_id=0, raw=False):
    """--dec --yuv-out: every code file becomes one frame of the raw .yuv file `path`, in the order of the list"""
    t1, _, model_idx, mse = _decoder_for(code_list, model_idx, mse, device_id, raw)
    for k, fc in enumerate(code_list):
        rec, geometry = _decode_file(t1, fc, model_idx, mse, height, width, raw, to_source=False)
        h, w = geometry.content
        yuv.write_frames(path, _rgb_yuv(rec, h, w, yuv_opts), h, w, yuv_opts["fmt"], append=k > 0)
        print('Decoding {}, output to {} frame {}'.format(fc, path, k))


def decoding_and_test_yuv(code_list, path, height, width, yuv_opts, start=0, model_idx=0, mse=True, device_id=0,
                          raw=False, ws=False, ms_ssim=False):
    """--test --yuv: decoding_and_test against frames start.. of a raw .yuv file.  The viewport figures (and with
    ws=True WS-PSNR / WS-SSIM) compare the converted source with the reconstruction, both cropped to the frame's own
    size; ws=True also prints WS-PSNR-Y/U/V of the frame as --dec --yuv-out would write it against the source frame.
    Rows: (bpp, vpsnr, vssim[, ws_psnr, ws_ssim, ws_psnr_y, ws_psnr_u, ws_psnr_v[, ws_ms_ssim]]): the last with
    ms_ssim=True (--ms-ssim), the WS-MS-SSIM of the pair WS-SSIM is taken of"""
    t1, dev, model_idx, mse = _decoder_for(code_list, model_idx, mse, device_id, raw)
    metrics = ViewportMetrics(device_id)
    frames = yuv.read_frames(path, height, width, yuv_opts["fmt"], start, len(code_list))
    rows = []
    for k, fc in enumerate(code_list):
        rec, geometry = _decode_file(t1, fc, model_idx, mse, height, width, raw, to_source=False)
        h, w = geometry.content
        if (h, w) != (height, width):
            raise ValueError("%s holds a %dx%d frame, --size says %dx%d" % (fc, w, h, width, height))
        src = frames[k:k + 1].to(dev)
        data, rdata = geometry.from_coded(_yuv_rgb(src, h, w, yuv_opts, dev)), geometry.from_coded(rec)
        pr, vssim = metrics(data, rdata)
        rt = bitrate(fc, *geometry.source)
        rows.append((rt, pr, vssim))
        print(('Decoding {}, compare it to {} frame {} \n ' + _VIEWPORT).format(fc, path, start + k, rt, pr, vssim))
        if ws:
            wmse, wssim = sphere_metrics.metrics(data, rdata)[0].tolist()
            back = _rgb_yuv(rec, h, w, yuv_opts).to(dev)
            rows[-1] += (sphere_metrics.psnr(wmse), wssim) + tuple(yuv.ws_psnr_yuv(src, back, h, w, yuv_opts["fmt"])[0].tolist())
            print(' ' + _WS.format(*rows[-1][3:5]))
            print(' ' + _WS_YUV.format(*rows[-1][5:]))
            if ms_ssim:
                rows[-1] += (sphere_metrics.ws_ms_ssim(data, rdata)[0].item(),)
                print(' ' + _WS_MS.format(rows[-1][-1]))
    return _report(rows, ([_VIEWPORT, _WS, _WS_YUV] + [_WS_MS] * bool(ms_ssim)) if ws else [_VIEWPORT])


def _parse_wxh(parser, flag, text):
    """(height, width) of a WIDTHxHEIGHT flag value; anything else ends the run with a message (parser.error)"""
    try:
        width, height = (int(v) for v in text.lower().split("x"))
    except ValueError:
        parser.error("%s takes WIDTHxHEIGHT, for example 3840x1920; got %r" % (flag, text))
    return height, width


def _yuv_flags(parser, args):
    """the checks of --yuv / --yuv-out / --pix-fmt; returns (height, width, options of yuv.to_rgb / from_rgb) or
    None when the call has nothing to do with YUV.  Contradictions end the run with a message (parser.error)"""
    if args.yuv is None and args.yuv_out is None:
        for flag, value in (("--pix-fmt", args.pix_fmt), ("--size", args.size), ("--frames", args.frames),
                            ("--start", args.start), ("--yuv-matrix", args.yuv_matrix), ("--yuv-range", args.yuv_range)):
            if value is not None:
                parser.error("%s needs --yuv or --yuv-out" % flag)
        return None
    if args.pix_fmt is None:
        parser.error("--yuv and --yuv-out need --pix-fmt (one of %s)" % ", ".join(sorted(yuv.FORMATS)))
    if args.rd:
        parser.error("--rd takes images (--img-list / --img-file), not --yuv")
    if args.native_size:
        parser.error("--native-size is for images: a YUV frame is always coded at its own size")
    if args.yuv is not None:
        if args.img_list is not None or args.img_file is not None:
            parser.error("--yuv and --img-list / --img-file are two sources for the same frames: give one")
        if not (args.enc or args.test):
            parser.error("--yuv is the source of --enc or --test; --dec writes to --yuv-out")
        if args.size is None:
            parser.error("--yuv needs --size WxH: a raw file does not carry its frame size")
    if args.yuv_out is not None:
        if not args.dec:
            parser.error("--yuv-out needs --dec")
        if args.out_list is not None or args.out_file is not None:
            parser.error("--yuv-out and --out-list / --out-file are two destinations for the same frames: give one")
        if args.start is not None or args.frames is not None:
            parser.error("--start and --frames select frames of --yuv; --dec writes one frame per code file")
    height = width = None
    if args.size is not None:
        height, width = _parse_wxh(parser, "--size", args.size)
        if height < 2 or width < 2 or height % 2 or width % 2:
            parser.error("--size %s: a 4:2:0 frame needs even sides of at least 2" % args.size)
    if args.frames is not None and args.code_list is not None and args.frames != len(args.code_list):
        parser.error("--frames %d but %d code files: one code file per frame" % (args.frames, len(args.code_list)))
    if (args.start or 0) < 0:
        parser.error("--start must not be negative")
    return height, width, dict(fmt=args.pix_fmt, matrix=args.yuv_matrix or "bt709", range=args.yuv_range or "limited")


def _code_size_flag(parser, args):
    """(H2, W2) of --code-size WxH, or None; contradictions end the run with a message (parser.error)"""
    if args.code_size is None:
        return None
    height, width = _parse_wxh(parser, "--code-size", args.code_size)
    if height < 2 or width < 2 or height > 1 << 20 or width > 1 << 20:
        parser.error("--code-size %s: each side must be in 2 .. 2^20" % args.code_size)
    if args.yuv is not None or args.yuv_out is not None:
        parser.error("--code-size is for images: the YUV path at a reduced size is not supported")
    if not (args.enc or args.rd):
        parser.error("--code-size goes with --enc or --rd; --dec and --test read the sizes from the file")
    if args.native_size:
        parser.error("--code-size and --native-size are two answers to the same question: give one")
    if args.enc and not (args.container and not args.raw):
        parser.error("--code-size needs --container: a headerless file cannot carry the two sizes")
    return height, width


def _rotate_flag(parser, args):
    """the integer triple of --rotate YAW,PITCH,ROLL (degrees), or None; contradictions end the run with a message
    (parser.error)"""
    if args.rotate is None:
        return None
    from . import erp_rotate
    try:
        yaw, pitch, roll = (float(v) for v in args.rotate.split(","))
    except ValueError:
        parser.error("--rotate takes YAW,PITCH,ROLL in degrees, for example 30,-45,0; got %r" % args.rotate)
    try:
        rotation = erp_rotate.units(yaw, pitch, roll)
    except erp_rotate.PconvError as exc:
        parser.error("--rotate %s: %s (yaw and roll in [-180, 180), pitch in [-90, 90])" % (args.rotate, exc))
    if args.yuv is not None or args.yuv_out is not None:
        parser.error("--rotate is for images: the YUV path converts and pads in one kernel and does not rotate")
    if not (args.enc or args.rd or args.test):
        parser.error("--rotate goes with --enc, --rd or --test; --dec reads the rotation from the file")
    if args.enc and not (args.container and not args.raw):
        parser.error("--rotate needs --container: a headerless file cannot carry the rotation")
    return rotation


def _projection_flag(parser, args):
    """the cube.Spec of --projection cmp|eac [--cube-layout faces|6x1|3x2], or None; contradictions end the run with a
    message"""
    if args.projection is None:
        if args.cube_layout is not None:
            parser.error("--cube-layout goes with --projection")
        return None
    from . import cube
    if args.yuv is not None or args.yuv_out is not None:
        parser.error("--projection is for images: the YUV path converts and pads in one kernel and takes no cube picture")
    if args.dec:
        parser.error("--projection goes with --enc, --rd or --test; --dec reads the projection from the file")
    if args.enc and not (args.container and not args.raw):
        parser.error("--projection needs --container: a headerless file cannot carry the projection")
    if args.native_size:
        parser.error("--projection excludes --native-size: a cube picture is always taken at its own size")
    return cube.spec(args.projection, args.cube_layout or "3x2")


def _cube_metrics_flag(parser, args, projection):
    """the checks of --cube-metrics: it goes with --projection on --test or --rd"""
    if args.cube_metrics:
        if projection is None:
            parser.error("--cube-metrics goes with --projection: it scores cube pictures as cube pictures")
        if not (args.test or args.rd) or args.enc or args.dec:
            parser.error("--cube-metrics goes with --test or --rd")
    return args.cube_metrics


def _cube_ssim_flag(parser, args, projection):
    """the checks of --cube-ssim, those of --cube-metrics: it goes with --projection on --test or --rd"""
    if args.cube_ssim:
        if projection is None:
            parser.error("--cube-ssim goes with --projection: it scores cube pictures as cube pictures")
        if not (args.test or args.rd) or args.enc or args.dec:
            parser.error("--cube-ssim goes with --test or --rd")
    return args.cube_ssim


def _view_flags(parser, args):
    """the checks of --view / --view-size / --view-out[-file] and --vp; returns (view, view size, vp): view the four
    angles in degrees or None, view size (vh, vw) or None, vp None, True (the default size) or (vh, vw).  Contradictions
    end the run with a message (parser.error)"""
    from . import viewport
    view = size = vp = None
    named = args.view_out is not None or args.view_out_file is not None
    if args.view is None:
        for flag, given in (("--view-size", args.view_size is not None), ("--view-out", named)):
            if given:
                parser.error("%s needs --view YAW,PITCH,ROLL,HFOV" % flag)
    else:
        try:
            view = tuple(float(v) for v in args.view.split(","))
            if len(view) != 4:
                raise ValueError
        except ValueError:
            parser.error("--view takes YAW,PITCH,ROLL,HFOV in degrees, for example 30,-45,0,90; got %r" % args.view)
        if not args.dec:
            parser.error("--view goes with --dec: it writes a view of every decoded picture (--test / --rd: --vp)")
        if args.yuv is not None or args.yuv_out is not None:
            parser.error("--view is for images: the YUV path stops at the coded frame")
        if args.view_size is None or not named:
            parser.error("--view needs --view-size WxH and --view-out (or --view-out-file)")
        if args.view_out is not None and args.view_out_file is not None:
            parser.error("--view-out and --view-out-file are two lists of the same names: give one")
        size = _parse_wxh(parser, "--view-size", args.view_size)
        try:
            viewport.view(*view, size=size)
        except viewport.PconvError as exc:
            parser.error("--view %s --view-size %s: %s (yaw and roll in [-180, 180), pitch in [-90, 90], hfov and the "
                         "vfov of square pixels in [1, 170], sides of 2 .. 2^20)" % (args.view, args.view_size, exc))
    if args.vp is not None:
        if not (args.test or args.rd) or args.enc or args.dec:
            parser.error("--vp goes with --test or --rd")
        if args.yuv is not None or args.yuv_out is not None:
            parser.error("--vp is for images: with --yuv the viewport figures stay those of the first line")
        vp = True
        if args.vp != "":
            vp = _parse_wxh(parser, "--vp", args.vp)
            if not all(2 <= v <= 1 << 20 for v in vp):
                parser.error("--vp %s: each side must be in 2 .. 2^20" % args.vp)
    return view, size, vp


def _sphere_flag(parser, args):
    """the checks of --sphere: it goes with --test or --rd, on images"""
    if args.sphere:
        if not (args.test or args.rd) or args.enc or args.dec:
            parser.error("--sphere goes with --test or --rd")
        if args.yuv is not None or args.yuv_out is not None:
            parser.error("--sphere is for images: the 4:2:0 planes of --yuv are not sampled on the sphere")
    return args.sphere


def read_list(fname):
    with open(fname) as f:
        return [line.rstrip('\n') for line in f.readlines()]


def check_models():
    assert os.path.exists('{}/{}_encoder.pt'.format(mse_model_dir, model_mse_list[0])), \
        'Please make sure the pretrained models for VMSE exists in the mse_model_dir'
    assert os.path.exists('{}/{}_encoder.pt'.format(ssim_model_dir, model_ssim_list[0])), \
        'Please make sure the pretrained models for VSSIM exists in the ssim_model_dir'


def main(argv=None):
    parser = argparse.ArgumentParser(description='Pseudo Convolution for 360 Image Compression')
    parser.add_argument('--img-list', nargs='*', help='The image list contains the input images for encoding and testing')
    parser.add_argument('--code-list', nargs='*', help='The code file list for codes')
    parser.add_argument('--out-list', nargs='*', help='The out list for saving decoded images.')
    parser.add_argument('--img-file', help='The file contains the input images for encoding and testing')
    parser.add_argument('--code-file', help='The file contains the list for codes')
    parser.add_argument('--out-file', help='The file  contains the names of decoded images.')
    parser.add_argument('--model-idx', type=int, default=0, help='Model index (0-9) for VMSE, (0-8) for VSSIM')
    parser.add_argument('--enc', action='store_true', default=False, help='Encoding flag, set for encoding phase.')
    parser.add_argument('--dec', action='store_true', default=False, help='Decoding flag, set for decoding phase.')
    parser.add_argument('--test', action='store_true', default=False, help='Testing flag, set for decoding and evalating the performance.')
    parser.add_argument('--rd', action='store_true', default=False,
                        help='Rate-distortion flag: score the images without writing code files (rate from the CDF '
                             'tables, reconstruction from the encoder\'s own symbols).  Takes --img-list/--img-file only')
    parser.add_argument('--ssim', action='store_true', default=False,
                        help='Default with models optimized for VMSE, set this flag for choosing the models optimized for VSSIM')
    parser.add_argument('--gpu-id', type=int, default=0, help='The graphic card id for encoding and decoding.')
    parser.add_argument('--height', type=int, default=512, help='ERP height of the coded image (multiple of 256)')
    parser.add_argument('--width', type=int, default=1024, help='ERP width of the coded image (multiple of 16)')
    parser.add_argument('--container', action='store_true', default=False,
                        help='Encoding: put a 16-byte header (size, model, valid_dim, length) in front of the stream, so '
                             "that the file decodes without --height/--width/--model-idx/--ssim.  Default: the reference's "
                             'headerless files.  Decoding recognises such files by their magic')
    parser.add_argument('--native-size', action='store_true', default=False,
                        help='Encoding: code every image at its own size (any height and width, no resize; '
                             '--height/--width are ignored): the frame is padded at the poles and the seam to '
                             'the next codable size and the decoder crops back.  Needs --container '
                             '(--rd: needs nothing, no file is written)')
    parser.add_argument('--code-size', help='Encoding / --rd: WIDTHxHEIGHT to code every image at, whatever its own size: '
                                            'the picture is resized on the device by the sphere-aware Lanczos-3 rule '
                                            '(seam wrapped, poles continued), the file records both sizes, --dec and '
                                            '--test work at the source size and the bitrate counts the source\'s '
                                            'pixels.  Needs --container (--rd: nothing), excludes --native-size')
    parser.add_argument('--rotate', help='Encoding / --rd / --test: YAW,PITCH,ROLL in degrees (yaw and roll in [-180, 180), '
                                         'pitch in [-90, 90]): code every image in the orientation that puts the point at '
                                         'longitude YAW, latitude PITCH in the centre of the picture, where the codec '
                                         'spends the most samples; the file records the angles, --dec turns the picture '
                                         'back and --test / --rd score against the unrotated source.  Needs --container '
                                         '(--rd: nothing; --test: checks that the files record these angles)')
    parser.add_argument('--projection', choices=['cmp', 'eac'],
                        help='Encoding / --rd / --test: the images are cube pictures, plain (cmp) or equi-angular (eac), '
                             'taken at their own size; they are converted on the device to the ERP frame of twice by four '
                             'times the face size and the file records kind, layout and face size (container version 5); '
                             '--dec writes the cube picture back.  Needs --container on --enc; not for --yuv')
    parser.add_argument('--cube-layout', choices=['faces', '6x1', '3x2'],
                        help='The layout of the cube pictures of --projection (default 3x2: L F R over D B U)')
    parser.add_argument('--cube-metrics', action='store_true', default=False,
                        help='Testing (--test / --rd) with --projection: after CUBE-PSNR also report CUBE-WS-PSNR (every '
                             'cube pixel weighted by its solid angle) and CUBE-S-PSNR-NN / CUBE-S-PSNR-I / CUBE-CPP-PSNR: '
                             'the original cube picture against the reconstructed one, both read as cube pictures at the '
                             'same points of the sphere, with no conversion to ERP in between')
    parser.add_argument('--cube-ssim', action='store_true', default=False,
                        help='Testing (--test / --rd) with --projection: after every other cube line also report '
                             'CUBE-WS-SSIM, the SSIM of the original cube picture against the reconstructed one with every '
                             'face continued from its neighbours by the radius of the SSIM window and every pixel weighted '
                             'by its solid angle.  Independent of --cube-metrics')
    parser.add_argument('--raw', action='store_true', default=False,
                        help='Decoding: never look for a container header (size and model from the flags)')
    parser.add_argument('--ws', action='store_true', default=False,
                        help='Testing: also report WS-PSNR / WS-SSIM (rows weighted by their area on the sphere) of '
                             'each decoded image at its own size.  Needs --test or --rd')
    parser.add_argument('--ms-ssim', action='store_true', default=False,
                        help='Testing: with --ws, also report WS-MS-SSIM (five scales of 2x2 means, sphere-weighted '
                             'per scale) of each decoded image; images of at least 16 x 16')
    parser.add_argument('--view', help='Decoding: YAW,PITCH,ROLL,HFOV in degrees: also write the rectilinear view of every '
                                       'decoded picture that looks at longitude YAW, latitude PITCH with a horizontal '
                                       'field of view HFOV (1 .. 170) and square pixels, anti-aliased (viewport.py).  '
                                       'Needs --view-size and --view-out')
    parser.add_argument('--view-size', help='WIDTHxHEIGHT of the views of --view')
    parser.add_argument('--view-out', nargs='*', help='The names of the views of --view, one per code file')
    parser.add_argument('--view-out-file', help='The file contains the names of the views of --view')
    parser.add_argument('--vp', nargs='?', const='', help='Testing (--test / --rd): also report VP-PSNR / VP-SSIM, the plain '
                                                          'PSNR / SSIM of 14 anti-aliased rectilinear views of '
                                                          'WIDTHxHEIGHT (default: a quarter of the picture\'s width, 3:2) '
                                                          'rendered from each picture at its own size')
    parser.add_argument('--sphere', action='store_true', default=False,
                        help='Testing (--test / --rd): also report S-PSNR-NN, S-PSNR-I (an icosphere of 655 362 points) and '
                             'CPP-PSNR: both pictures sampled at the same points of the sphere.  A file coded with '
                             '--code-size gets a second line, the source against the reconstruction at the coded size, '
                             'with no resize in between')
    parser.add_argument('--yuv', help='Encoding / testing: a raw YUV 4:2:0 file as the source instead of images, one '
                                      'code file per frame (needs --size and --pix-fmt)')
    parser.add_argument('--yuv-out', help='Decoding: write the decoded frames to this raw YUV 4:2:0 file, in the order '
                                          'of the code list (needs --pix-fmt; --size for headerless code files)')
    parser.add_argument('--size', help='WIDTHxHEIGHT of the frames of --yuv (any even size: padded at the poles and the seam)')
    parser.add_argument('--pix-fmt', choices=sorted(yuv.FORMATS), help='Pixel format of --yuv / --yuv-out')
    parser.add_argument('--frames', type=int, help='Frames to read from --yuv (default: one per code file)')
    parser.add_argument('--start', type=int, help='First frame to read from --yuv (default 0)')
    parser.add_argument('--yuv-matrix', choices=sorted(yuv.MATRICES), help='YCbCr matrix (default bt709)')
    parser.add_argument('--yuv-range', choices=sorted(yuv.RANGES), help='Code value range (default limited)')
    args = parser.parse_args(argv)
    code_size = _code_size_flag(parser, args)
    rotation = _rotate_flag(parser, args)
    projection = _projection_flag(parser, args)
    cube_metrics = _cube_metrics_flag(parser, args, projection)
    cube_ssim = _cube_ssim_flag(parser, args, projection)
    view, view_size, vp = _view_flags(parser, args)
    sphere = _sphere_flag(parser, args)
    yuv_call = _yuv_flags(parser, args)   # contradictory YUV flags end the run here, before anything is loaded
    assert not args.ws or ((args.test or args.rd) and not args.enc and not args.dec), '--ws needs --test or --rd'
    assert not args.ms_ssim or args.ws, '--ms-ssim needs --ws'
    assert not args.rd or not (args.enc or args.dec or args.test), '--rd excludes --enc, --dec and --test'
    check_models()
    midx = args.model_idx
    if args.ssim:
        assert 0 <= midx < 9, '(0-8) for VSSIM'
    else:
        assert 0 <= midx < 10, '(0-9) for VMSE'
    assert args.enc or args.dec or args.test or args.rd, \
        'Should set one flag, (--enc) for encoding, (--dec) for decoding, (--test) for testing, (--rd) for scoring.'
    pick = lambda lst, fil: lst if lst is not None else (read_list(fil) if fil is not None else None)
    img_list, code_list, out_list = pick(args.img_list, args.img_file), pick(args.code_list, args.code_file), \
        pick(args.out_list, args.out_file)
    size = dict(height=args.height, width=args.width)
    if yuv_call is not None:
        height, width, yuv_opts = yuv_call
        assert code_list is not None, 'No code files'
        assert args.frames is None or args.frames == len(code_list), 'One code file per frame: --frames differs from the code list'
        common = dict(model_idx=midx, mse=not args.ssim, device_id=args.gpu_id)
        if args.enc:
            encoding_yuv(args.yuv, code_list, height, width, yuv_opts, start=args.start or 0,
                         boxed=args.container and not args.raw, **common)
        elif args.dec:
            decoding_yuv(code_list, args.yuv_out, yuv_opts, height, width, raw=args.raw, **common)
        else:
            decoding_and_test_yuv(code_list, args.yuv, height, width, yuv_opts, start=args.start or 0, raw=args.raw,
                                  ws=args.ws, ms_ssim=args.ms_ssim, **common)
    elif args.rd:
        assert img_list is not None, 'No input images for scoring'
        rate_distortion(img_list, midx, not args.ssim, args.gpu_id, native=args.native_size, ws=args.ws,
                        code_size=code_size, rotation=rotation, ms_ssim=args.ms_ssim, vp=vp, sphere=sphere,
                        projection=projection, cube_metrics=cube_metrics, cube_ssim=cube_ssim, **size)
    elif args.enc:
        assert img_list is not None, 'No input images for encoding'
        assert code_list is not None, 'No code files for saving the codes'
        assert len(img_list) == len(code_list), 'The number of images and codes should be the same'
        assert not args.native_size or (args.container and not args.raw), '--native-size needs --container'
        encoding(img_list, code_list, midx, not args.ssim, args.gpu_id, boxed=args.container and not args.raw,
                 native=args.native_size, code_size=code_size, rotation=rotation, projection=projection, **size)
    else:
        assert code_list is not None, 'No code files for decoding'
        if args.dec:
            assert out_list is not None, 'No out files for saving the decoded images'
            assert len(code_list) == len(out_list), 'The number of codes and reconstructed images should be the same'
            view_list = pick(args.view_out, args.view_out_file)
            assert view is None or len(view_list) == len(code_list), 'The number of codes and views should be the same'
            decoding(code_list, out_list, midx, not args.ssim, args.gpu_id, raw=args.raw, view=view, view_size=view_size,
                     view_list=view_list, **size)
        else:
            assert img_list is not None, 'No source images for evaluation.'
            assert len(code_list) == len(img_list), 'The number of codes and corresponding source images should be the same'
            decoding_and_test(code_list, img_list, midx, not args.ssim, args.gpu_id, raw=args.raw, ws=args.ws,
                              rotation=rotation, ms_ssim=args.ms_ssim, vp=vp, sphere=sphere, projection=projection,
                              cube_metrics=cube_metrics, cube_ssim=cube_ssim, **size)


if __name__ == '__main__':
    main()
