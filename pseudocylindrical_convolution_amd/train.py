"""End-to-end training of the codec, one process per GPU over RCCL
(reference: test/trainDDP_Full.py; test/trainDDP_Base.py is the same loop with --base).

    python -m pseudocylindrical_convolution_amd.train --gpus 8 --data-dir ... --train-list ... --test-list ...
    python -m torch.distributed.run --nproc-per-node 8 -m pseudocylindrical_convolution_amd.train ...

The loop, the loss (gamma*viewport MSE + beta*(1 - viewport SSIM) + alpha*rate; with `--loss ws` the two
viewport terms become the sphere-weighted WS-MSE and WS-SSIM of sphere_metrics.loss_terms, with `--loss ws-ms`
WS-MSE and WS-MS-SSIM of sphere_metrics.ms_loss_terms, with `--loss vp` the MSE and SSIM of the 14 anti-aliased views
of viewport.py that --test --vp reports: viewport.loss_terms, through the renderer's ordered backward), the alternating
optimisers (entropy model / transforms + quantiser levels, the histogram "gradient" of `quant.count`
applied by its own SGD), gradient accumulation over `acc_batch` steps with clipping, and the
checkpoint naming follow the reference.  What differs: ranks come from the launcher's environment
(RANK / LOCAL_RANK / WORLD_SIZE) instead of mp.spawn, every path is an argument, and
`--synthetic N` / `--procedural N` train on generated images where no dataset exists, and
`--time-budget S` ends the run after S seconds of wall time (the epoch in flight stops at its next
step, is tested and saved as usual), and `--deterministic` trains on the ordered (atomic-free) backward kernels
(PCONV.ordered_backward) under torch's deterministic settings and logs the parameter checksum two runs from one
seed are compared on, and `--conv native` keeps the 1x1 / 3x3 convolutions on this project's kernels, forward and
backward (PCONV.native_conv_grad), and `--conv native-all` the entropy model's masked 5x5 convolutions too
(PCONV.native_masked_conv), with the SSIM term of --loss viewport computed by sphere_metrics.loss_terms(uniform): no
convolution of a training step is the vendor library's then, and `--optim native` takes the step of the two Adam
optimisers (accumulated gradient, global norm, clip, update) to optim.Adam, whose every operation include/pconv_hip.h
defines.  The whole state of a run is written to `<prefix>_state.pt` at the end of every epoch and at an early stop
(`--time-budget`, `--stop-after N` batches); `--resume` continues from it at the recorded epoch and batch and ends
with the bits of the run that was never interrupted (optim.TrainState).  `--code-size WxH` trains the reduced-size
pipeline that `--test --code-size` scores: the batch is resized down (erp_resample.resize, clamped), the model runs at
the coded size, its output is resized back under autograd (the resize's ordered backward) and every loss reads the
frames at the source size; the rate counts bits over the source's pixels."""
from __future__ import print_function

import argparse
import contextlib
import os
import sys
import time
from itertools import chain

import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel as DDP

from . import PCONV, erp_resample, erp_size, model_zoo_v2, optim, sphere_metrics, viewport
from .PCONV_operator import Logger, ModuleSaver, MultiProject, SSIM, backend
from .RDMetric import mse_tb
from .SphereDataset import (ProceduralSphereDataSet, SphereDataSet, SyntheticSphereDataSet,
                            load_train_test_distribute)
from .model_zoo_v2 import AccGrad

SPHERE_LOSSES = {'ws': sphere_metrics.loss_terms, 'ws-ms': sphere_metrics.ms_loss_terms}   # --loss: read the ERP frames

OWN_LOSSES = tuple(SPHERE_LOSSES) + ('vp', 'cube-ws')   # --loss: no MultiProject, no SSIM module; test() scores by the loss itself
_vp_renderers = {}   # (h, w, device, --vp-size) -> viewport.Renderer of the 14 paper views


def vp_size(text):
    """--vp-size WxH -> (vh, vw)"""
    try:
        vw, vh = (int(v) for v in text.lower().split('x'))
    except ValueError:
        raise argparse.ArgumentTypeError('--vp-size is WxH, e.g. 256x171, got {!r}'.format(text))
    return vh, vw


def code_size(text):
    """--code-size WxH -> (h2, w2); a size the codec does not take as it is (erp_size.codable) is refused"""
    try:
        w2, h2 = (int(v) for v in text.lower().split('x'))
    except ValueError:
        raise argparse.ArgumentTypeError('--code-size is WxH, e.g. 1024x512, got {!r}'.format(text))
    if not erp_size.codable(h2, w2):
        raise argparse.ArgumentTypeError('--code-size {}x{}: the model codes widths that are multiples of {} and heights '
                                         'that are multiples of {}'.format(w2, h2, erp_size.COLS, erp_size.TILE_ROWS))
    return h2, w2


class _Parser(argparse.ArgumentParser):
    """the checks that need two arguments at once are parser errors too"""

    def parse_args(self, args=None, namespace=None):
        ns = super(_Parser, self).parse_args(args, namespace)
        if ns.code_size is not None:
            for name, n_in, n_out in (('height', ns.height, ns.code_size[0]), ('width', ns.width, ns.code_size[1])):
                if max(n_in, n_out) > erp_resample.MAX_SHRINK * min(n_in, n_out):   # the way there, or the way back
                    self.error('--code-size: a {} of {} -> {} shrinks by more than {}:1 on the way there or back'.format(
                        name, n_in, n_out, erp_resample.MAX_SHRINK))
        return ns


def vp_renderer(args, data):
    """the renderer of --loss vp for frames like `data`: the 14 paper directions (viewport.paper_views) at --vp-size, by
    default at the size --test --vp scores at (ViewportScore: vw = w // 4, vh = (2 vw + 1) // 3), anti-aliased by
    viewport.plan; one per frame size and device, its maps built once.  prefilter_grad: a view that plan renders from a
    reduced source (more than 4 source pixels per view pixel) carries its gradient through the resize's ordered backward"""
    h, w = data.shape[2:]
    key = (h, w, str(data.device), getattr(args, 'vp_size', None))
    if key not in _vp_renderers:
        size = key[3] if key[3] is not None else ((2 * (w // 4) + 1) // 3, w // 4)
        _vp_renderers[key] = viewport.Renderer(h, w, viewport.paper_views(size), size, device=data.device,
                                               prefilter_grad=True)
    return _vp_renderers[key]


def cube_ws_terms(args, data, y):
    """the two distortion terms of --loss cube-ws, float64 (n,) each: cube.ws_loss_terms (the solid-angle weighted squared
    error) and cube.ws_ssim_loss_terms (the cube WS-SSIM that --cube-ssim reports) of cube.from_erp(y) against
    cube.from_erp(data), a --cube-kind picture ("3x2") of face size --cube-face, by default cube.face_size(h, w).  The
    target is data: it is converted under no_grad.  The gradient reaches y through the ordered backwards of the weighted
    metrics, of the face continuation and of from_erp's renderer"""
    from . import cube
    kind, a = getattr(args, 'cube_kind', None), getattr(args, 'cube_face', None)
    a = cube.face_size(*data.shape[2:]) if a is None else a
    sp = cube.spec(kind or 'cmp', '3x2')
    with torch.no_grad():
        target = cube.from_erp(data, a, sp)
    picture = cube.from_erp(y, a, sp)
    return cube.ws_loss_terms(target, picture, sp), cube.ws_ssim_loss_terms(target, picture, sp)


def get_params(model, ent):
    m = model.module
    if ent:
        return m.ent.parameters()
    return chain(m.encoder.parameters(), m.decoder.parameters(), [m.quant.weight])


def forward_losses(args, model, data, pr1, pr2, sim_func):
    """(mse, ssim, rate) of one batch; rate is None for the base model.  --loss viewport: MSE and SSIM over the 14
    projected views; --loss ws: the batch means of WS-MSE and WS-SSIM over the ERP frames themselves (pr1, pr2 and
    sim_func are None); --loss ws-ms: the same with WS-MS-SSIM in the place of WS-SSIM; --loss vp: the batch means of
    viewport.loss_terms, the MSE and SSIM of the 14 anti-aliased views of viewport.py that --test --vp reports, the
    gradient through the renderer's ordered backward (pr1, pr2 and sim_func are None).  --loss viewport without a
    sim_func (--conv native-all): the SSIM term is sphere_metrics.loss_terms(uniform) over the views -- pytorch_ssim's
    map (the 11-tap sigma 1.5 window, zero padding of 5, its C1 and C2) on this project's kernels; all views have one
    size, so the mean of the frame means is the mean of the map.  --code-size: the chain of FrameGeometry.to_coded /
    from_coded -- the model sees the batch resized to the coded size (clamped; no gradient: it is data), its output comes
    back to the source size through erp_resample.resize under autograd (clamped), every distortion term reads the
    frames at the source size, and the rate per coded pixel is scaled by (h2 w2) / (h w): bits over the source's pixels"""
    coded = getattr(args, 'code_size', None)
    out = model(data if coded is None else erp_resample.resize(data, coded[0], coded[1], clamp=True))
    y, ent_vec, mask = out if isinstance(out, tuple) else (out, None, None)
    if coded is not None:
        y = erp_resample.resize(y, data.shape[2], data.shape[3], clamp=True)
    if args.loss in SPHERE_LOSSES:
        terms = SPHERE_LOSSES[args.loss](data, y)
        mse, ssim = terms[:, 0].mean(), terms[:, 1].mean()
    elif args.loss == 'vp':
        terms = viewport.loss_terms(vp_renderer(args, data), data, y)
        mse, ssim = terms[:, 0].mean(), terms[:, 1].mean()
    elif args.loss == 'cube-ws':
        mse, ssim = (t.mean() for t in cube_ws_terms(args, data, y))
    else:
        py, px = pr1(y), pr2(data)
        mse = torch.mean((px - py) * (px - py))
        if sim_func is None:
            ssim = sphere_metrics.loss_terms(px, py, weighting="uniform")[:, 1].mean()
        else:
            ssim = sim_func(px, py)
    rate = None if ent_vec is None else torch.sum(ent_vec) / torch.sum(mask).item()
    if rate is not None and coded is not None:
        rate = rate * (float(coded[0] * coded[1]) / float(data.shape[2] * data.shape[3]))
    return mse, ssim, rate


def make_sim_func(args, device):
    """the SSIM module of the viewport loss; None where forward_losses needs none: the sphere-weighted losses, --loss
    vp, and --conv native-all (SSIM(11, 3) blurs with the library's convolution and is not constructed there)"""
    if args.loss in OWN_LOSSES or getattr(args, 'conv', 'vendor') == 'native-all':
        return None
    return SSIM(11, 3).to(device)


def should_stop(args, run, device):
    """whether the run ends here: the time budget is used up, or --stop-after batches are trained.  With more than
    one rank it is rank 0's answer, broadcast, that every rank acts on -- a deadline read per rank would let one rank
    leave the loop for the checksum all-reduce while another enters the next batch's gradient all-reduce.  Every rank
    asks at the same places: before each batch and before each epoch."""
    deadline, after = getattr(args, 'deadline', None), getattr(args, 'stop_after', 0)
    if not deadline and not after:
        return False
    stop = bool(deadline and time.monotonic() >= deadline) or bool(after and run.global_batch >= after)
    if run.world_size > 1:
        flag = torch.tensor([int(stop)], dtype=torch.int32, device=device)
        dist.broadcast(flag, 0)
        stop = bool(flag.item())
    return stop


def train(args, model, device, train_loader, optimizer, optimizer_quant, epoch, log, pr1, pr2, ent=True, run=None):
    """one epoch (reference: trainDDP_Full.py:21-56), or what is left of it: with run.next_batch > 0 (a resumed run,
    optim.TrainState) the sampler yields the epoch's order from that batch on, the accumulators start from the saved
    ones, and the loader's iterator is made from the random state the epoch began with.  Sets run.stopped where
    should_stop ended the epoch early; run.next_batch is then the batch a resumed run starts at."""
    run = run if run is not None else optim.TrainState()
    model.train()
    train_loader.sampler.set_epoch(epoch)
    acc_grad = AccGrad(get_params(model, ent))
    start = run.next_batch if run.epoch == epoch else 0
    if start:
        train_loader.sampler.skip = start * args.batch_size
        for a, saved in zip(acc_grad.acc_grad, run.acc):
            a.copy_(saved)
        optim.rng_set(run.rng_epoch, device)
    else:
        run.rng_epoch = optim.rng_get(device)
    run.epoch, run.next_batch, run.acc = epoch, start, None
    batches = enumerate(train_loader, start)   # the loader draws its seeds here
    if start:
        optim.rng_set(run.rng, device)
    native_step = isinstance(optimizer, optim.Adam)
    sim_func = make_sim_func(args, device)
    gamma, beta, alpha, clip = args.gamma, args.beta, args.alpha, args.clip
    log.log('clip:{}'.format(clip))
    acc_batch = args.acc_batch
    last = run.last if start else None
    for batch_idx, data in batches:
        if not data.shape[0] == args.batch_size:
            run.next_batch = batch_idx + 1
            continue
        if args.max_steps and batch_idx >= args.max_steps:
            break
        if should_stop(args, run, device):
            run.stopped = True
            break
        data = data.to(device)
        optimizer.zero_grad()
        optimizer_quant.zero_grad()
        mse_loss, ssim, ent_loss = forward_losses(args, model, data, pr1, pr2, sim_func)
        ssim_loss = 1 - ssim
        loss = gamma * mse_loss + beta * ssim_loss
        if ent_loss is not None:
            loss = loss + alpha * ent_loss
        loss.backward()
        optimizer_quant.step()
        param = list(get_params(model, ent))
        if batch_idx % acc_batch == acc_batch - 1 and native_step:
            # copy_back, clip_grad_norm_ and Adam.step in the three launches of csrc/optim.hip (include/pconv_hip.h)
            optimizer.step(acc=acc_grad.acc_grad, clip=clip)
        elif batch_idx % acc_batch == acc_batch - 1:
            acc_grad.copy_back(param)
            if clip > 0:
                torch.nn.utils.clip_grad_norm_(param, clip)
            optimizer.step()
        else:
            acc_grad.acc(param)
        last = (loss.item(), mse_loss.item(), 1 - ssim_loss.item(), float('nan') if ent_loss is None else ent_loss.item())
        log.log('Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f} mse:{:.6f} ssim:{:.3} rate:{:.3}'.format(
            epoch, batch_idx * len(data), len(train_loader.dataset), 100. * batch_idx / len(train_loader), *last))
        run.global_batch, run.next_batch = run.global_batch + 1, batch_idx + 1
    run.acc, run.last = acc_grad.acc_grad, last
    return last


def test(args, model, device, test_loader, log, pr1, pr2):
    """viewport MSE / SSIM / rate over the test set, scored against the anchor curve
    (reference: trainDDP_Full.py:58-86).  --loss ws / ws-ms / vp: the loss's own MSE / SSIM / rate, scored by the training loss itself
    (the anchor curve is one of viewport MSE)"""
    model.eval()
    sim_func = make_sim_func(args, device)
    test_mse, test_ssim, test_ent, n = 0., 0., 0., 0
    vd = args.valid_dim / 256. * .815
    for data in test_loader:
        with torch.no_grad():
            mse, ssim, rate = forward_losses(args, model, data.to(device), pr1, pr2, sim_func)
        test_mse += mse.item()
        test_ssim += ssim.item()
        test_ent += 0. if rate is None else rate.item()
        n += 1
    test_mse, test_ssim, test_ent = test_mse / max(n, 1), test_ssim / max(n, 1), test_ent / max(n, 1)
    if args.base:
        log.log('\nTest set: MSE loss: {:.6f}  ssim loss: {:.4f}'.format(test_mse, test_ssim))
        rt_loss = [args.gamma * test_mse + args.beta * (1 - test_ssim)]
    else:
        real_rt = vd * test_ent / 0.693
        log.log('\nTest set: MSE loss: {:.6f}  ssim loss: {:.4f} Ent: {:.3f} rt: {:.3f}bpp'.format(
            test_mse, test_ssim, test_ent, real_rt))
        if args.loss in OWN_LOSSES:
            rt_loss = [args.gamma * test_mse + args.beta * (1 - test_ssim) + args.alpha * test_ent]
        else:
            rt_loss = [float(test_mse - mse_tb(real_rt))]
    log.log(('tloss: ' + '{}\t' * len(rt_loss)).format(*rt_loss))
    return rt_loss


def init_with_trained_model(path, model, device):
    """copy every tensor of the checkpoint whose name exists in the model (reference: :93-100)"""
    pdict = torch.load(path, map_location=device)
    ndict = model.state_dict()
    for key in ndict.keys():
        if key in pdict.keys():
            ndict[key] = pdict[key]
    model.load_state_dict(ndict)


def setup(rank, world_size, backend):
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '12355')
    dist.init_process_group(backend=backend, rank=rank, world_size=world_size)


def make_datasets(args):
    if args.procedural:
        ntest = max(args.test_batch_size, min(8, args.procedural // 8))
        train_data = ProceduralSphereDataSet(args.procedural, args.height, args.width, seed=args.seed * 2 + 1)
        test_data = ProceduralSphereDataSet(ntest, args.height, args.width, seed=args.seed * 2 + 2)
        return train_data, test_data, train_data.values()
    if args.synthetic:
        ntest = max(args.test_batch_size, args.synthetic // 8)
        train_data = SyntheticSphereDataSet(args.synthetic, args.height, args.width, seed=1)
        test_data = SyntheticSphereDataSet(ntest, args.height, args.width, seed=2)
        return train_data, test_data, train_data.values()
    train_data = SphereDataSet(True, args.data_dir, args.train_list)
    test_data = SphereDataSet(False, args.data_dir, args.test_list)
    return train_data, test_data, args.values


@contextlib.contextmanager
def deterministic_mode():
    """what --deterministic sets, put back afterwards: this project's four float-atomic backward kernels give way to
    their ordered forms, and torch is asked for deterministic algorithms of its own (warn_only: an op of torch's
    that has none warns and runs)"""
    before = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark,
              torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    with PCONV.ordered_backward(True):
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
        torch.use_deterministic_algorithms(True, warn_only=True)
        try:
            yield
        finally:
            torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before[:2]
            torch.use_deterministic_algorithms(before[2], warn_only=before[3])


def native_conv_mode(conv='native'):
    """what --conv native / native-all sets, put back when the returned context ends: the convolutions of a training
    step (TileConv2d and the GDN's 1x1 contraction) stay on this project's kernels, forward and backward
    (PCONV.native_conv_grad); under native-all the entropy model's masked 5x5 convolutions as well
    (PCONV.native_masked_conv).  Refused on a backend that has no such kernels, before a switch is touched."""
    ops = backend.ops()
    kernels = ('tile_conv2d_backward', 'conv5x5_backward') if conv == 'native-all' else ('tile_conv2d_backward',)
    if not all(hasattr(ops, name) for name in kernels):
        raise RuntimeError('--conv {} needs the HIP backend: {} has no convolution backward kernels '
                           '({}); use --conv vendor'.format(conv, getattr(ops, '__name__', ops), ', '.join(kernels)))
    switches = contextlib.ExitStack()
    switches.enter_context(ops.native_conv_grad(True))
    if conv == 'native-all':
        switches.enter_context(ops.native_masked_conv(True))
    return switches


def native_all_conv_mode():
    return native_conv_mode('native-all')


def Job(rank, world_size, args):
    """what one rank does (reference: trainDDP_Full.py:102-163)"""
    conv = getattr(args, 'conv', 'vendor')
    native = conv in ('native', 'native-all')
    if native and args.device != 'cuda':
        raise RuntimeError('--conv {} needs --device cuda: the convolution backward kernels are HIP kernels; '
                           'use --conv vendor'.format(conv))
    with native_conv_mode(conv) if native else contextlib.nullcontext():
        if getattr(args, 'deterministic', False):
            with deterministic_mode():
                return _job(rank, world_size, args)
        return _job(rank, world_size, args)


def _job(rank, world_size, args):
    deterministic = getattr(args, 'deterministic', False)
    on_gpu = args.device == 'cuda'
    cid = int(os.environ.get('LOCAL_RANK', rank)) if (on_gpu and not args.share_gpu) else 0
    args.gpu_id = cid
    torch.manual_seed(args.seed)  # same initial weights on every rank; DDP broadcasts rank 0's anyway
    setup(rank, world_size, args.dist_backend or ('nccl' if on_gpu else 'gloo'))
    device = torch.device('cuda:%d' % cid) if on_gpu else torch.device('cpu')
    if on_gpu:
        torch.cuda.set_device(device)
    train_data, test_data, values = make_datasets(args)
    train_loader, test_loader = load_train_test_distribute(
        world_size, rank, args.batch_size, args.test_batch_size, mean=args.mean, acc_batch=args.acc_batch,
        train_data=train_data, test_data=test_data, values=values, num_workers=args.workers)
    save_dir = os.path.join(args.base_dir, 'save_models')
    if rank == 0:
        os.makedirs(save_dir, exist_ok=True)
    dist.barrier()
    prex = '{}_{}_{}_{}_{}'.format('base' if args.base else 'ent', 'opt' if args.opt else 'normal', args.channels,
                                   args.valid_dim, args.npart)
    prex = '{}_init'.format(prex) if args.init else prex
    resume = getattr(args, 'resume', None)
    state_path = '{}/{}_state.pt'.format(save_dir, prex)
    log = Logger('{}/{:s}_logs_{}.txt'.format(save_dir, prex, cid), screen=args.verbose and rank == 0, file=(rank == 0),
                 append=resume is not None)
    if args.loss in OWN_LOSSES:
        pr1 = pr2 = None  # the sphere-weighted loss reads the ERP frames themselves, --loss vp renders its own views
    else:
        vs = args.viewport_size
        pr1 = MultiProject(vs, int(vs * 1.5), 0.5, False, cid).to(device)
        pr2 = MultiProject(vs, int(vs * 1.5), 0.5, False, cid).to(device)
    net_class = model_zoo_v2.CMPNetV2M if args.base else model_zoo_v2.CMPNetV2MF
    model = net_class(args.valid_dim, args.channels, args.code_dim, args.npart, opt=args.opt, init=args.init,
                      device_id=cid)
    saver = ModuleSaver(save_dir + '/', prex) if rank == 0 else None
    wrap = lambda m: DDP(m.to(device), [cid] if on_gpu else None)
    best, latest = '{}/{}_best_0.pt'.format(save_dir, prex), '{}/{}_latest.pt'.format(save_dir, prex)
    if resume is not None:
        model = wrap(model)   # weights, best losses and everything else come from the state file, below
    elif args.init:
        # stage 2 trains the entropy model on top of the stage-1 transforms: an own checkpoint of this
        # stage, else --init-from, else what `--base` wrote (trainDDP_Full.py:118-122 loads
        # save_models/base_opt_192_{valid_dim}_16_best_0.pt).  Never from random transforms.
        base_best = '{}/base_{}_{}_{}_{}_best_0.pt'.format(save_dir, 'opt' if args.opt else 'normal', args.channels,
                                                           args.valid_dim, args.npart)
        of = best if os.path.exists(best) else (args.init_from or base_best)
        if not os.path.exists(of) and not args.init_random:
            raise FileNotFoundError(
                '--init needs the stage-1 transforms: no checkpoint at {} (run --base first or pass --init-from; '
                '--init-random trains on random transforms, for smoke runs only)'.format(of))
        if os.path.exists(of):
            init_with_trained_model(of, model, device)
            log.log('load init model {} successful...'.format(of))
        else:
            log.log('WARNING: --init-random: no stage-1 checkpoint at {}, the entropy model is trained on RANDOM transforms'.format(of))
        model = wrap(model)
    elif os.path.exists(best):
        of = latest if (args.latest and os.path.exists(latest)) else best
        init_with_trained_model(of, model, device)
        model = wrap(model)
        ls = test(args, model, device, test_loader, log, pr1, pr2)
        if args.restart:
            ls = [1e9 for _ in range(len(ls))]
        if rank == 0:
            saver.init_loss(ls)
        log.log('load model successful...')
    else:
        of = args.init_from or '{}/{}_init_best_0.pt'.format(save_dir, prex)
        if os.path.exists(of):
            init_with_trained_model(of, model, device)
            log.log('initialize the model with {}...'.format(of))
        else:
            log.log('no checkpoint at {}: training from random weights'.format(of))
        model = wrap(model)
    optimizer_quant = torch.optim.SGD([model.module.quant.count], lr=0.001)
    native_optim = getattr(args, 'optim', 'torch') == 'native'
    Adam = optim.Adam if native_optim else torch.optim.Adam
    optimizer_other = Adam([{'params': model.module.encoder.parameters()},
                            {'params': model.module.decoder.parameters()},
                            {'params': [model.module.quant.weight]}], lr=args.lr)
    optimizer_ent = None if args.base else Adam(model.module.ent.parameters(), lr=args.lr * 10)
    optimizers = {'other': optimizer_other, 'ent': optimizer_ent, 'quant': optimizer_quant}
    run = optim.TrainState()
    if resume is not None:
        run = optim.TrainState.load(resume or state_path, args, world_size, model.module, optimizers, saver,
                                    train_loader.sampler, device)
        log.log('resumed from {}: epoch {}, batch {}, {} batches trained so far'.format(
            resume or state_path, run.epoch, run.next_batch, run.global_batch))
    run.world_size = world_size

    def save_state():
        if rank == 0:
            run.save(state_path, args, world_size, model.module, optimizers, saver, train_loader.sampler, device)

    log.log('lr:{}'.format(args.lr))
    if deterministic:
        log.log('deterministic: ordered backward kernels {}, cudnn.deterministic {}, cudnn.benchmark {}, '
                'torch deterministic algorithms {} (warn only), optimiser step {}{}'.format(
                    'on' if PCONV.backward_is_ordered() else 'off', torch.backends.cudnn.deterministic,
                    torch.backends.cudnn.benchmark, torch.are_deterministic_algorithms_enabled(),
                    'native (optim.Adam, in the order of include/pconv_hip.h)' if native_optim else "torch's",
                    '' if not PCONV.conv_grad_is_native() else
                    ', convolutions native, incl. the masked 5x5 and the viewport SSIM' if PCONV.masked_conv_is_native() else
                    ', convolutions native' + (
                        '' if args.loss in OWN_LOSSES else
                        ' (not the 11x11 blur of the viewport loss\'s SSIM, which stays the library\'s: --loss ws / ws-ms have none)')))
    if args.loss in SPHERE_LOSSES:
        log.log('loss: WS-MSE / {} over the ERP frames (--viewport_size is ignored)'.format(
            'WS-SSIM' if args.loss == 'ws' else 'WS-MS-SSIM'))
    if args.loss == 'vp':
        log.log('loss: MSE / SSIM over the 14 anti-aliased views of viewport.py at {} (--viewport_size is ignored)'.format(
            'the size of --test --vp (a quarter of the width)' if getattr(args, 'vp_size', None) is None else
            '{}x{}'.format(args.vp_size[1], args.vp_size[0])))
    if args.loss == 'cube-ws':
        log.log('loss: WS-MSE / WS-SSIM over the {} cube picture of the frames, faces of {} (--viewport_size is ignored)'.format(
            getattr(args, 'cube_kind', None) or 'cmp',
            'cube.face_size(h, w)' if getattr(args, 'cube_face', None) is None else args.cube_face))
    if getattr(args, 'code_size', None) is not None:
        log.log('code size: the model runs at {}x{}; losses and rate are those of the frames at their own size'.format(
            args.code_size[1], args.code_size[0]))
    log.log('valid dims:{} \t alpha:{}'.format(args.valid_dim, args.alpha))
    history = run.history   # of a resumed run: the epochs finished before it
    args.deadline = time.monotonic() + args.time_budget if args.time_budget > 0 else None
    for epoch in range(run.epoch, args.epochs + 1):
        if should_stop(args, run, device):
            log.log('time budget of {} s used up or --stop-after {} reached: {} batches trained, {} epoch(s) begun'.format(
                args.time_budget, getattr(args, 'stop_after', 0), run.global_batch, epoch - 1))
            break
        if args.base or (not args.init and epoch % 4 == 1):
            last = train(args, model, device, train_loader, optimizer_other, optimizer_quant, epoch, log, pr1, pr2, False, run)
        else:
            last = train(args, model, device, train_loader, optimizer_ent, optimizer_quant, epoch, log, pr1, pr2, True, run)
        if run.stopped:
            # the state of the stop itself, before the evaluation below that the uninterrupted run never makes: the
            # resumed run finds the best losses, the random generators and the history of the finished epochs
            save_state()
        ls = test(args, model, device, test_loader, log, pr1, pr2)
        history.append((last, ls))
        if rank == 0:
            log.log(saver.save(model, ls))
        if not run.stopped:
            run.epoch, run.next_batch, run.acc, run.last = epoch + 1, 0, None, None
            save_state()
    if world_size > 1 or deterministic:
        # the ranks end with the same parameters (DDP averaged every gradient): spread of a checksum over the ranks
        # (--deterministic: the figure two runs from one seed are compared on, one rank included)
        chk = torch.zeros(1, dtype=torch.float64, device=device)
        for p in model.module.parameters():
            chk += p.detach().double().abs().sum()
        hi, lo = chk.clone(), chk.clone()
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        log.log('parameter checksum over {} ranks: {:.9e}, spread {:.3e}'.format(world_size, hi.item(), (hi - lo).item()))
    dist.barrier()
    dist.destroy_process_group()
    return history


def build_parser():
    parser = _Parser(description='PyTorch 360 Compression (MI355X)')
    parser.add_argument('--gpus', type=int, default=0,
                        help='start this many ranks on this node (0: ranks come from the launcher environment)')
    parser.add_argument('--device', default='cuda', choices=['cuda', 'cpu'],
                        help='cpu = gloo ranks on the test backend (tests only)')
    parser.add_argument('--batch-size', type=int, default=4, metavar='N')
    parser.add_argument('--acc-batch', type=int, default=3)
    parser.add_argument('--test-batch-size', type=int, default=4, metavar='N')
    parser.add_argument('--epochs', type=int, default=30, metavar='N')
    parser.add_argument('--lr', type=float, default=0.0001, metavar='LR')
    parser.add_argument('--valid-dim', type=int, default=192)
    parser.add_argument('--gamma', type=float, default=1, help='trade-off of MSE loss')
    parser.add_argument('--beta', type=float, default=0, help='trade-off of SSIM loss')
    parser.add_argument('--alpha', type=float, default=1, help='trade-off of rate loss')
    parser.add_argument('--clip', type=float, default=0.1,
                        help='global gradient-norm clip per optimiser step; 0 = none.  (The reference passes an exhausted '
                             'generator to clip_grad_norm_, trainDDP_Full.py:43-46, so its runs are in effect unclipped: '
                             'use --clip 0 to reproduce them)')
    parser.add_argument('--opt', action='store_true', default=True, help='optimised tile split')
    parser.add_argument('--no-opt', dest='opt', action='store_false')
    parser.add_argument('--init', action='store_true', default=False,
                        help='first stage: train the entropy model only, its gradient cut off from the codes')
    parser.add_argument('--base', action='store_true', default=False,
                        help='the transforms only, no entropy model (trainDDP_Base.py)')
    parser.add_argument('--latest', action='store_true', default=False)
    parser.add_argument('--restart', action='store_true', default=False)
    parser.add_argument('--cube-kind', default=None, choices=['cmp', 'eac'],
                        help='the cube projection of --loss cube-ws (default: cmp)')
    parser.add_argument('--cube-face', type=int, default=None, metavar='A',
                        help='the face size of --loss cube-ws (default: cube.face_size(h, w), a quarter of the width)')
    parser.add_argument('--loss', default='viewport', choices=['viewport', 'ws', 'ws-ms', 'vp', 'cube-ws'],
                        help='distortion terms: viewport = MSE and SSIM over 14 rectilinear views (the paper\'s loss); '
                             'ws = WS-MSE and WS-SSIM over the ERP frame (sphere_metrics.loss_terms: what --test --ws '
                             'reports); ws-ms = WS-MSE and WS-MS-SSIM (sphere_metrics.ms_loss_terms: --test --ws --ms-ssim); '
                             'vp = MSE and SSIM over the 14 paper directions rendered by viewport.py, anti-aliased, at a '
                             'size that follows the frame (viewport.loss_terms: what --test --vp reports; the gradient '
                             'runs through the renderer\'s ordered, atomic-free backward, and for a view of more than 4 '
                             'source pixels per view pixel through that of the resize in front of it); '
                             'cube-ws = the solid-angle weighted squared error and the cube WS-SSIM (what --cube-ssim '
                             'reports) of the output and the frame, both converted to a --cube-kind cube picture of face '
                             'size --cube-face (cube.ws_loss_terms, cube.ws_ssim_loss_terms).  '
                             'gamma, beta and alpha weigh the terms alike; with ws, ws-ms, vp and cube-ws the best checkpoint is '
                             'the one with the lowest gamma*mse + beta*(1 - ssim) + alpha*rate on the test set')
    parser.add_argument('--vp-size', type=vp_size, default=None, metavar='WxH',
                        help='size of a view of --loss vp (default: that of --test --vp, W = width // 4, H = (2 W + 1) // 3: '
                             '256x171 at 1024 columns)')
    parser.add_argument('--code-size', type=code_size, default=None, metavar='WxH',
                        help='train the reduced-size pipeline of --test --code-size: the batch is resized to WxH '
                             '(erp_resample.resize), the model runs there, its output is resized back under autograd and '
                             'every loss reads the frames at their own size; the rate is bits over the source\'s pixels.  '
                             'WxH must be a size the model codes as it is, and no more than 8:1 below --width x --height')
    parser.add_argument('--viewport_size', type=int, default=171, metavar='viewport',
                        help='side of a projected view (ignored with --loss ws, ws-ms and vp)')
    parser.add_argument('--channels', type=int, default=192)
    parser.add_argument('--code-dim', type=int, default=192)
    parser.add_argument('--npart', type=int, default=16)
    parser.add_argument('--mean', type=float, default=1.5, help="the sampler's minimum mean image value per step")
    parser.add_argument('--base-dir', default='.', help='checkpoints and logs go to <base-dir>/save_models')
    parser.add_argument('--init-from', default=None, help='checkpoint to initialise from')
    parser.add_argument('--init-random', action='store_true', default=False,
                        help='--init without a stage-1 checkpoint: go on from random transforms (smoke runs only)')
    parser.add_argument('--data-dir', default='./360_512')
    parser.add_argument('--train-list', default=None)
    parser.add_argument('--test-list', default=None)
    parser.add_argument('--values', default=None, help='pickle: image name -> value, for the balanced sampler')
    parser.add_argument('--synthetic', type=int, default=0, help='train on this many generated images')
    parser.add_argument('--procedural', type=int, default=0,
                        help='train on this many procedural images (gradients, textures, hard-edged shapes)')
    parser.add_argument('--time-budget', type=float, default=0,
                        help='stop after this many seconds of wall time (0: run all epochs)')
    parser.add_argument('--height', type=int, default=512)
    parser.add_argument('--width', type=int, default=1024)
    parser.add_argument('--workers', type=int, default=4)
    parser.add_argument('--max-steps', type=int, default=0, help='stop an epoch after this many batches (0: all)')
    parser.add_argument('--dist-backend', default=None, choices=['nccl', 'gloo'],
                        help='default: nccl (RCCL) on the GPU, gloo on the CPU.  gloo with --device cuda = several ranks on ONE '
                             'GPU (RCCL refuses two ranks per device): a rehearsal of the DDP path, not a deployment')
    parser.add_argument('--share-gpu', action='store_true', default=False,
                        help='every rank on cuda:0 (with --dist-backend gloo): rehearsal on a one-GPU box')
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--deterministic', action='store_true', default=False,
                        help='reproducible training: the ordered (atomic-free) forms of the slice, uslice, viewport and '
                             'quantiser backward kernels (PCONV.ordered_backward), cudnn.deterministic, no cudnn benchmark, '
                             'torch.use_deterministic_algorithms(True, warn_only=True); logs the parameter checksum to '
                             'compare two runs on.  Guaranteed for this project\'s own kernels; the vendor library\'s '
                             'convolution backward is outside it (--conv native replaces it for the 1x1 / 3x3 layers, '
                             '--conv native-all for every convolution of a training step)')
    parser.add_argument('--conv', default='vendor', choices=['vendor', 'native', 'native-all'],
                        help='whose kernels the convolutions of a training step run on.  vendor: the library behind '
                             'torch (forward and backward).  native: this project\'s fp32-MFMA kernels, the backward in '
                             'the defined order of include/pconv_hip.h (PCONV.native_conv_grad) -- every 1x1 / 3x3 '
                             'convolution of the transforms and the GDN.  Two convolutions stay with the library: the '
                             'entropy model\'s masked 5x5 ones, and the 11x11 blur of the SSIM term of --loss viewport '
                             '(--loss ws / ws-ms have none: with them the --base stage reaches no library convolution).  '
                             'native-all: as native, and the masked 5x5 convolutions on this project\'s kernels too '
                             '(PCONV.native_masked_conv: the dense fmaf chain on the masked weight), and the SSIM term '
                             'of --loss viewport by sphere_metrics.loss_terms(uniform) -- the same 11-tap window on this '
                             'project\'s kernels -- in the place of pytorch_ssim\'s SSIM(11, 3): no configuration reaches '
                             'a library convolution.  native and native-all: HIP backend only')
    parser.add_argument('--optim', default='torch', choices=['torch', 'native'],
                        help='whose arithmetic the two Adam optimisers\' step is.  torch: AccGrad.copy_back, clip_grad_norm_ '
                             'and torch.optim.Adam.step.  native: optim.Adam -- the accumulated gradient, its global norm '
                             '(a two-stage fp64 sum of fixed shape), the clip and the update in three launches of '
                             'csrc/optim.hip, every operation defined in include/pconv_hip.h; on --device cpu its twin in '
                             'numpy, bit for bit the same.  The state layout is torch\'s: a state file of one loads into the '
                             'other (not under --resume, which refuses a changed --optim like any other changed argument)')
    parser.add_argument('--resume', nargs='?', const='', default=None, metavar='PATH',
                        help='continue the run whose state PATH holds (default: <base-dir>/save_models/<prefix>_state.pt, '
                             'written at the end of every epoch and when --time-budget or --stop-after stops a run): model, '
                             'optimisers, epoch and batch, gradient accumulators, the quantiser\'s call counters, best losses, '
                             'sampler and random generators.  The resumed run ends with the bits of the uninterrupted one.  '
                             'Refused, naming the argument, when an argument that shapes the trajectory differs (all but '
                             '--epochs, --time-budget, --stop-after, --resume, --verbose, --workers, --base-dir) or the world '
                             'size does; a missing file is an error.  Not held equal: the evaluation at an early stop may '
                             'write a _best_ checkpoint of a moment the uninterrupted run never evaluates')
    parser.add_argument('--stop-after', type=int, default=0, metavar='N',
                        help='stop when N batches are trained over the whole run, resumed parts included, exactly as a '
                             'time budget that ran out there (0: no such stop)')
    parser.add_argument('--verbose', action='store_true', default=False)
    return parser


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    if args.gpus > 0 and 'WORLD_SIZE' not in os.environ:
        # become the launcher: one child per GPU through torch.distributed.run
        import subprocess
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
               '--master-addr', '127.0.0.1', '--master-port', os.environ.get('MASTER_PORT', '29517'),
               '-m', 'pseudocylindrical_convolution_amd.train'] + argv
        return subprocess.call(cmd)
    rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    Job(rank, world, args)
    return 0


if __name__ == '__main__':
    sys.exit(main())
