"""One data-parallel training iteration of the fusion head (BASELINE.json
configs[2]: batch-per-GPU 1, DDP, gradient all-reduce over RCCL/xGMI).

What the reference does per iteration (tools/train.py -> mmcv EpochBasedRunner
-> MMDistributedDataParallel + OptimizerHook, CFG:206-221):
forward -> loss dict -> sum -> backward -> bucketed NCCL all-reduce of the
2.6 M trainable gradients -> clip_grad_norm_(35) -> AdamW step.  Here:

  * the trainable, used parameters live in ONE flat fp32 buffer and their
    gradients in another (parameters and .grad are views): the whole gradient
    exchange is a single all-reduce of 10.5 MB, issued on the
    RCCL stream by torch.distributed (backend "nccl" = RCCL on ROCm);
  * sum-of-squares, clip coefficient, 1/world_size and the AdamW update run on
    the flat buffers in two HIP kernels (tc_sq_norm, tc_adamw_step) -- the clip
    coefficient never leaves the device, so the step has no host sync;
  * the packed weights of the fused forward chains are refreshed in place.
"""
import ctypes as C
import math

import torch
import torch.distributed as dist

from . import _lib as L
from .detr3d_head import MATRIX_PATHS, SEED_STRIDE, head_options, radar_table


def exchange_chunk_of(name, num_fusion_layers=3):
    """Chunk of the gradient exchange a trainable parameter of the fusion stack belongs to, in the order the backward
    finishes the weight gradients (tc_radar_train_bwd_weights).  With N = num_fusion_layers: 0 .. N - 1 = fusion layer
    N .. 1 (HEAD:129-171: the modules with suffix `3` / `_3`, `2` / `_2`, none), N = the radar encoders and anything else
    -- N + 1 chunks.  The default depth of 3: 0 / 1 / 2 = fusion layer 3 / 2 / 1, 3 = the encoders."""
    n = L.check_num_fusion_layers(num_fusion_layers)
    head = name.split('.')[0]
    stems = ('final_cls', 'final_reg', 'rf_multihead_attn', 'rf_linear1', 'rf_linear2', 'rf_norm1', 'rf_norm2', 'rf_norm3')
    for stem in stems:
        if head.startswith(stem):
            tail = head[len(stem):]
            layer = 2 if tail in ('3', '_3') else 1 if tail in ('2', '_2') else 0 if tail == '' else None
            if layer is not None and layer < n:
                return n - 1 - layer
    return n


class FlatBucket:
    """Flat parameter / gradient storage for [(name, parameter)].

    chunk_of (round 6): name -> chunk index.  The parameters of a chunk are stored contiguously, chunk 0 first
    (``chunk_ranges``: [(begin, end)] element ranges): the gradient exchange can then travel chunk by chunk while the
    backward is still producing the next one (``all_reduce_chunk_begin``).  ``names`` / ``items`` / ``offsets`` stay in
    the order of ``named_params``."""

    def __init__(self, named_params, chunk_of=None):
        self.names = [n for n, _ in named_params]
        self.items = [p for _, p in named_params]
        if not self.items:
            raise ValueError('no trainable parameters')
        chunks = [int(chunk_of(n)) if chunk_of is not None else 0 for n in self.names]
        order = sorted(range(len(self.items)), key=lambda i: (chunks[i], i))
        dev = self.items[0].device
        n = sum(p.numel() for p in self.items)
        self.params = torch.empty(n, dtype=torch.float32, device=dev)
        # one allocation: the gradients and, behind them, the squared-norm slots of the clip (tc_sq_norm: one per
        # workgroup, added up in index order by tc_adamw_step; zeroed by the same fill)
        self._store = torch.zeros(n + L.TC_SQ_NORM_PARTIALS, dtype=torch.float32, device=dev)
        self.grads = self._store[:n]
        self.sq = self._store[n:]
        self.offsets = [0] * len(self.items)
        self.chunk_ranges = []
        off = 0
        for i in order:
            p = self.items[i]
            k = p.numel()
            self.params[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.params[off:off + k].view(p.shape)
            p.grad = self.grads[off:off + k].view(p.shape)
            self.offsets[i] = off
            if not self.chunk_ranges or chunks[i] != self._last_chunk:
                self.chunk_ranges.append([off, off])
                self._last_chunk = chunks[i]
            off += k
            self.chunk_ranges[-1][1] = off
        self.chunk_ranges = [tuple(r) for r in self.chunk_ranges]
        self.numel = n

    def zero_grad(self, check_views=True):
        self._store.zero_()
        if not check_views:          # nobody re-bound a .grad since the last call (the fused iteration)
            return
        for p, off in zip(self.items, self.offsets):     # a None grad would detach the view
            if p.grad is None or p.grad.data_ptr() != self.grads.data_ptr() + 4 * off:
                p.grad = self.grads[off:off + p.numel()].view(p.shape)

    def all_reduce(self):
        """SUM over ranks, one collective for the whole bucket."""
        return self.all_reduce_end(self.all_reduce_begin())

    def all_reduce_begin(self):
        """Start the bucket's ONE all-reduce (SUM) without waiting for it: ordered behind everything already enqueued on
        the current stream (the backward's weight-gradient kernel), it runs on the backend's communication stream
        (RCCL) beside whatever other streams have in flight -- the look-ahead of the frozen decoder.  -> handle."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return dist.all_reduce(self.grads, op=dist.ReduceOp.SUM, async_op=True), dist.get_world_size()
        return None, 1

    def all_reduce_chunk_begin(self, i):
        """Start the all-reduce (SUM) of chunk i alone -- ordered behind what is enqueued on the current stream (the launch
        that produced the chunk's last gradients), beside whatever the compute stream does next (the next chunk's weight
        gradients).  -> (handle or None, world size), for ``all_reduce_end``."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            a, b = self.chunk_ranges[i]
            return dist.all_reduce(self.grads[a:b], op=dist.ReduceOp.SUM, async_op=True), dist.get_world_size()
        return None, 1

    @staticmethod
    def all_reduce_end(pending):
        """The current stream (not the host, on RCCL) waits for the exchange -- one handle or a list of chunk handles, in
        the order they were started; -> world size."""
        world = 1
        for work, w in (pending if isinstance(pending, list) else [pending]):
            if work is not None:
                work.wait()
            world = w
        return world


def cosine_lr(base_lr, cur_iter, cur_epoch, max_epochs, warmup_iters=4000, warmup_ratio=1.0 / 3,
              min_lr_ratio=1e-3):
    """CFG:216-221: mmcv CosineAnnealing (by epoch) with linear warm-up (by
    iteration) [3p-memory: mmcv.runner.hooks.lr_updater]."""
    target = base_lr * min_lr_ratio
    regular = target + 0.5 * (base_lr - target) * (1 + math.cos(math.pi * cur_epoch / max_epochs))
    if cur_iter < warmup_iters:
        k = (1 - cur_iter / warmup_iters) * (1 - warmup_ratio)
        return regular * (1 - k)
    return regular


def _g(t):
    return None if t is None or t.grad is None else C.c_void_p(t.grad.data_ptr())


def grad_table(head):
    """tc_head_weights whose pointers are the .grad buffers of the trainable stack's
    parameters (the table tc_radar_train_bwd adds into)."""
    g = L.tc_head_weights()
    g.abi_version = L.TC_ABI_VERSION
    return radar_table(head, g, _g)


class FusionTrainer:
    """head: transcar_amd.Detr3DHead on the GPU, built with ``train_cfg``."""

    #: coefficient of the forward counter in Detr3DHead.next_dropout_seed (detr3d_head.dropout_seed_of): consecutive
    #: training forwards draw seeds this far apart, which lets ONE launch give every frame of a look-ahead batch its masks
    SEED_STRIDE = SEED_STRIDE

    def __init__(self, head, lr=1.5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
                 max_norm=35.0, device_loss=True, dropout=0.1, seed=0, decoder_dropout=None,
                 chain_forward=True, chain_backward=True, prefetch_depth=1, deterministic=False):
        self.head = head.freeze_decoder()
        # deterministic=True (round 5): the fused backward accumulates order-free
        # (tc_radar_train_bwd_fused_det: integer atomics on a fixed-point shadow of the gradient bucket and of dK | dV) --
        # two runs from the same state give bit-identical gradients and parameters, on any schedule.  The default keeps
        # the float atomics (what torch's own backward does in the reference): bench.py --full --train reports both.
        self.deterministic = bool(deterministic)
        if self.deterministic and not chain_backward:
            raise ValueError('FusionTrainer(deterministic=True) needs the fused backward (chain_backward=True): the '
                             'per-operator backward (tc_radar_train_bwd) accumulates with float atomics')
        self._shadow = None
        # Round 6: the bucket is laid out in EXCHANGE CHUNKS -- fusion layer N, .., 1, radar encoders
        # (N = head.num_fusion_layers: N + 1 chunks),
        # the order in which the backward finishes their weight gradients -- and with more than one rank an iteration
        # launches the weight gradients chunk by chunk (tc_radar_train_bwd_weights) with one asynchronous all-reduce
        # behind each: chunk k travels while chunk k + 1 is computed (`chunked_exchange`; tools/train.py:253-260: DDP's
        # buckets).  One rank, or deterministic=True (the order-free backward flushes its shadow once, behind ONE grouped
        # launch): the single grouped launch and the single all-reduce of round 5.
        self.chunked_exchange = True
        depth = head.num_fusion_layers
        self.bucket = FlatBucket(head.trainable_parameters(), chunk_of=lambda name: exchange_chunk_of(name, depth))
        head.refresh_weights()                      # parameter addresses moved into the bucket
        self.m = torch.zeros_like(self.bucket.params)
        self.v = torch.zeros_like(self.bucket.params)
        self.sq = self.bucket.sq               # zeroed with the gradients (FlatBucket.zero_grad)
        # set by load_checkpoint alone, for a checkpoint of ANOTHER bucket layout: the clip's sum of squares is then taken
        # over the gradients in the layout of the run that is continued (`_adopt_clip_order`)
        self._clip_order = self._clip_index = self._clip_scratch = None
        self.lr, self.betas, self.eps = lr, betas, eps
        self.weight_decay, self.max_norm = weight_decay, max_norm
        self.iter = 0
        self.device_loss = device_loss     # step_fused_nhwc: losses + their gradients from HIP kernels
        # step_fused_nhwc: dropout of the fusion layers as the reference trains them (HEAD:129-171,
        # p = 0.1); counter-based masks from (seed, iteration).  The frozen decoder and the
        # per-operator autograd path (step / step_nhwc) run without dropout.
        self.dropout, self.seed = float(dropout), int(seed)
        head.dropout_seed = int(seed)
        # the frozen decoder's own dropouts (the reference leaves them active, tools/train.py:245-252):
        # None = as the modules are configured (0.1) when the fusion layers train with dropout, else off
        if decoder_dropout is None:
            decoder_dropout = head.decoder_dropout_p() if self.dropout > 0 else 0.0
        self.decoder_dropout = float(decoder_dropout)
        # step_fused_nhwc: the stack's forward as launches of the fused row chains with the tape stored as it
        # is produced (tc_radar_train_fwd_fused: 3 launches + 1 re-pack instead of ~66); False = the
        # operator-by-operator forward tc_radar_train_fwd (the same tape: the cross-check of the tests)
        self.chain_forward = bool(chain_forward)
        # ... and its backward as one launch of the backward row chain (query side), a handful for the token
        # side and one grouped weight-gradient launch (tc_radar_train_bwd_fused: ~16 launches instead of ~130);
        # False = tc_radar_train_bwd, one launch per operator
        self.chain_backward = bool(chain_backward)
        self._sq_clean = False
        # Look-ahead of the FROZEN decoder (tools/train.py:245-252: nothing an iteration trains feeds it).  1 = the next
        # frame's decoder forward runs on a side stream during this iteration (round 3: one frame, 4-row tiles, 0.44 ms
        # of a 1.0 ms iteration at 19 % of the matrix peak).  P > 1 (round 4): the decoder forwards of the next P
        # frames as ONE batched launch sequence (16-row tiles on the f16 matrix cores, the inference rate), every
        # frame with the dropout masks of its own seed (tc_head_options.dropout_seed_stride); the iterations then
        # consume the batch frame by frame.  The decoder's arithmetic is fixed by the depth, not by whether a frame
        # was prefetched (`decoder_tile_rows`): with P > 1 a frame that missed the look-ahead runs the same 16- / 32-row
        # kernels alone, so losses and parameters do not depend on the schedule.
        # Round 5: a look-ahead of more than 4 096 rows (nine frames: 8 100) runs the 32-row tiles, like inference.
        self.prefetch_depth = max(1, int(prefetch_depth))
        rows = self.prefetch_depth * int(head.num_query)
        self.decoder_tile_rows = max(16, L.chain_tile_rows(rows)) if self.prefetch_depth > 1 else None

        #: matrix path of the frozen decoder's forward (head_options(matrix_path=)): None / 'auto', 'f32', 'f16x2'
        self.decoder_matrix_path = None
        # the look-ahead: the batch in use and the one behind it (`prefetch_decoder`), its side stream; the head lane of
        # the decoder forward in use, the generation of `invalidate_lookahead`, frames taken from a look-ahead so far
        self._pre = self._pre_next = self._pre_stream = None
        self._lane = self._generation = self.lookahead_hits = 0
        # allocated anew when their key changes: tape and backward workspace (B, T), gradient table (bucket address)
        self._tape = self._tape_key = self._bws = self._bws_key = self._gtab = self._gtab_key = None
        self._wT_ready, self.last_dropout_seed = False, None
        #: keep_last = True: `_last` holds the operands of the last backward call (tests).  The three lists, when set,
        #: collect timing events (bench.py --full --train): per chunk's gradients, around the exchange wait, that per chunk
        self.keep_last, self._last = False, None
        self.chunk_events = self.exchange_events = self.exchange_chunk_events = None

    def _decoder_tile_rows_now(self):
        """`decoder_tile_rows`, resolved at the call: 32-row tiles exist on the f16x2 matrix path only, so with
        ``decoder_matrix_path = 'f32'`` -- or after the f16-range guard's fall-back -- a depth that asks for 32 rows
        runs the f32 kernels' 16 (Detr3DHead.effective_tile_rows).  A number or an unknown name: left to the library."""
        mp = MATRIX_PATHS.get(self.decoder_matrix_path)
        return self.head.effective_tile_rows(self.decoder_tile_rows, mp, derived=True)

    def _stream(self):
        return L.stream_ptr()

    def backward_and_step(self, losses, lr=None):
        """losses: dict from head.loss(); every key containing 'loss' is summed
        (mmdet BaseDetector._parse_losses)."""
        total = sum(v for k, v in losses.items() if 'loss' in k)
        self.bucket.zero_grad()
        total.backward()
        self._optimizer_step(lr)
        return total.detach()

    # ------------------------------------------------------------------
    # fast path: the trainable stack as two C calls (tc_radar_train_fwd / _bwd) instead of
    # ~160 autograd nodes; torch autograd only differentiates the loss itself
    # ------------------------------------------------------------------
    def _decoder_forward(self, feats_nhwc, lidar2img, img_hw, tokens, pad_mult, seed, lane, lookahead=False):
        """The frozen decoder (train mode) on B >= 1 frames.  lookahead: the frames are consumed one per iteration, frame
        b draws the masks of seed + b * SEED_STRIDE (the seed of the iteration that will take it).  An ordinary batch
        (B > 1 frames of ONE iteration) draws from one index space with the iteration's seed: with the stride, sample 1
        of iteration n would repeat the masks of sample 0 of iteration n + 1."""
        with torch.no_grad():
            return self.head.forward_nhwc(feats_nhwc, lidar2img, img_hw, tokens, pad_mult, aux='train',
                                          _allow_train=True, decoder_only=True, lane=lane,
                                          options=head_options(tile_rows=self._decoder_tile_rows_now(),
                                                               matrix_path=self.decoder_matrix_path,
                                                               decoder_dropout_p=self.decoder_dropout,
                                                               dropout_seed=seed,
                                                               dropout_seed_stride=self.SEED_STRIDE if lookahead else 0))

    def _input_key(self, feats_nhwc, lidar2img, tokens, pad_mult):
        # address, shape, the tensors' version counters AND this trainer's look-ahead generation.  The version counter
        # sees torch's in-place operators only: a loader that refills the same static tensors through this package's
        # raw-pointer kernels (ops.to_nhwc into a preallocated buffer, RadarRawStage.build, FramePipeline write hooks,
        # any ctypes tc_* call) must call ``invalidate_lookahead()`` -- it bumps the generation, and a pending
        # look-ahead of the old contents is dropped instead of handing their decoder states to the new frame
        return (self._generation,
                tuple((int(f.data_ptr()), int(f._version), tuple(f.shape)) for f in feats_nhwc),
                (int(lidar2img.data_ptr()), int(lidar2img._version)), (int(tokens.data_ptr()), int(tokens._version)),
                int(pad_mult), tuple(tokens.shape))

    def invalidate_lookahead(self):
        """The tensors handed to ``prefetch_decoder`` / ``step_fused_nhwc(prefetch=...)`` were rewritten in place by
        something torch's version counters do not see: pending look-ahead frames are stale."""
        self._generation += 1
        self._pre = self._pre_next = None

    def prefetch_decoder(self, feats_nhwc, lidar2img, img_hw, tokens, pad_mult, skip=0):
        """Enqueue the FROZEN decoder's forward of the NEXT iteration(s) now, on a side stream: it depends on nothing
        this iteration trains (tools/train.py:245-252 freezes it), so it runs while the host waits for the cost
        matrix and solves the Hungarian assignment (device idle otherwise: ~0.25 ms of a 1.5 ms iteration) and
        beside the backward.  The tensors hold the next P >= 1 frames (batch dimension P: a loader's look-ahead,
        collated); the following P calls of step_fused_nhwc pick their frame up when they are handed the
        corresponding slices (``feats[6 i : 6 i + 6]``, ``lidar2img[i : i + 1]``, ``tokens[i : i + 1]``), in order.
        The inputs must stay untouched until then.  The dropout seeds are those the P iterations would draw
        themselves: the forward counter is NOT advanced here but when a frame is consumed, and a look-ahead whose
        seeds no longer match the counter (another training forward came in between) is dropped.
        skip: frames of an earlier look-ahead still to be consumed before these (their iterations draw the seeds in
        between).  step_fused_nhwc(prefetch=...) calls this at the right moment."""
        head = self.head
        head.check_frame_nhwc(feats_nhwc, lidar2img)
        if not head.training:
            head.train()
        cur = torch.cuda.current_stream()
        if self._pre_stream is None:
            self._pre_stream = torch.cuda.Stream()
        P = int(lidar2img.shape[0])
        ncam = feats_nhwc[0].shape[0] // P
        counter0 = head._train_forwards + int(skip)
        seed0 = head.peek_dropout_seed(1 + int(skip))          # the seed of the training forward that takes frame 0
        pend = self._pre
        lane = 1 - (pend['lane'] if pend is not None else self._lane)
        self._pre_stream.wait_stream(cur)                      # inputs written on the current stream are complete
        with torch.cuda.stream(self._pre_stream):
            base = self._decoder_forward(feats_nhwc, lidar2img, img_hw, tokens, pad_mult, seed0, lane, lookahead=True)
            ev = torch.cuda.Event()
            ev.record(self._pre_stream)
        for t in base['aux'].values():
            if torch.is_tensor(t):
                t.record_stream(cur)                           # allocated on the side stream, consumed on this one
        keys = [self._input_key([f[ncam * i:ncam * (i + 1)] for f in feats_nhwc], lidar2img[i:i + 1], tokens[i:i + 1],
                                pad_mult) for i in range(P)]
        new = dict(keys=keys, seed0=seed0, counter0=counter0, base=base, ev=ev, lane=lane, next=0, count=P)
        if pend is not None and skip:
            self._pre_next = new                               # behind the frames of the look-ahead in use
        else:
            self._pre, self._pre_next = new, None

    def _take_prefetched(self, feats_nhwc, lidar2img, tokens, pad_mult):
        """-> (aux of this frame, its dropout seed) from the pending look-ahead, or None."""
        if self._pre is None:
            self._pre, self._pre_next = self._pre_next, None
        pre = self._pre
        if pre is None:
            return None
        head, i = self.head, pre['next']
        ok = (i < pre['count'] and head._train_forwards == pre['counter0'] + i and
              lidar2img.shape[0] == 1 and pre['keys'][i] == self._input_key(feats_nhwc, lidar2img, tokens, pad_mult))
        if not ok:
            self._pre = self._pre_next = None                  # stale: nothing was drawn from the seed counter for it
            return None
        if i == 0:
            torch.cuda.current_stream().wait_event(pre['ev'])
            self._lane = pre['lane']
        seed = head.next_dropout_seed()
        assert seed == (pre['seed0'] + i * self.SEED_STRIDE) & 0xFFFFFFFFFFFFFFFF
        aux = pre['base']['aux']
        out = dict(inter_states=aux['inter_states'][:, i:i + 1], inter_references=aux['inter_references'][:, i:i + 1],
                   last_box=aux['last_box'][i:i + 1])
        pre['next'] = i + 1
        if pre['next'] >= pre['count']:
            self._pre, self._pre_next = self._pre_next, None
        self.lookahead_hits += 1
        return out, seed

    def lookahead_pending(self):
        """Frames of look-ahead batches not consumed yet."""
        n = 0
        for pre in (self._pre, self._pre_next):
            if pre is not None:
                n += pre['count'] - pre['next']
        return n

    def step_fused_nhwc(self, feats_nhwc, lidar2img, img_hw, tokens, pad_mult, gt_bboxes_list,
                        gt_labels_list, lr=None, update=True, prefetch=None):
        """update=False stops after the backward: the gradients sit in the bucket.
        prefetch: dict(feats_nhwc, lidar2img, img_hw, tokens, pad_mult) of the NEXT iteration's frame -- or, with
        ``prefetch_depth`` P > 1, of the next P frames (batch dimension P): their frozen decoder forward is enqueued
        on a side stream once this iteration's cost matrix is on its way (``prefetch_decoder``), as ONE batched
        launch sequence; the following calls pick their frame up when they are handed the same tensors (the
        slices of the batch, in order).  A callable is called as ``prefetch(skip)`` (-> the dict) only when a look-ahead
        is started: the frames that follow the `skip` frames of the look-ahead still in use (P > 1: the next batch is
        started one iteration before the current one runs out)."""
        head, lib = self.head, L.lib()
        head.check_frame_nhwc(feats_nhwc, lidar2img)       # (a frame of another camera count: before the seed counter moves)
        if not head.training:                      # (Module.train() walks ~380 submodules: 0.7 ms of host time per call)
            head.train()
        if self.device_loss:
            from .device_loss import check_assign_status
            check_assign_status(head)              # a non-finite cost matrix of an earlier iteration: ValueError, as scipy
        got = self._take_prefetched(feats_nhwc, lidar2img, tokens, pad_mult)
        if got is not None:
            aux, drop_seed = got
        else:
            drop_seed = head.next_dropout_seed()   # (seed, rank, forward counter): shared with forward_train_nhwc
            aux = self._decoder_forward(feats_nhwc, lidar2img, img_hw, tokens, pad_mult, drop_seed,
                                        self._lane)['aux']
        w = head.head_weights()
        B, T = lidar2img.shape[0], tokens.shape[1]
        hs_last = aux['inter_states'][-1].contiguous()
        ref_last = aux['inter_references'][-1].contiguous()
        last_box = aux['last_box']
        key = (B, T)
        if self._tape_key != key:
            self._tape = L.device_bytes(tokens.device, lib.tc_radar_train_tape_bytes, C.byref(w), B, T)
            self._tape_key = key
        tape = self._tape
        Q = head.num_query
        NF = head.num_fusion_layers
        all_cls = torch.empty((NF, B, Q, head.cls_out_channels), dtype=torch.float32, device=tokens.device)
        all_box = torch.empty((NF, B, Q, head.code_size), dtype=torch.float32, device=tokens.device)
        self._wT_ready = False
        if self.chain_forward:
            # the packed (4x4x1) copy of the trainable weights for the CURRENT parameters -- and, when the backward is
            # the fused one too, its transposed packed weights in the same launch (the parameters do not change
            # between this forward and its backward): one launch instead of two
            pv = head._packed_view
            if self.chain_backward:
                bws = self._backward_workspace(lib, w, key, B, T, tokens.device)
                L.check(lib.tc_radar_train_repack(C.byref(w), C.byref(pv), bws.data_ptr(), bws.numel(), B, T,
                                                  L.stream_ptr()), 'tc_radar_train_repack')
                self._wT_ready = True
            else:
                L.check(lib.tc_head_repack_trainable_ex(C.byref(w), C.byref(pv), 1, L.stream_ptr()),
                        'tc_head_repack_trainable_ex')
            head._packed_dirty = True                  # the 16x16x4 copy (inference at >= 3 frames) is stale
            L.check(lib.tc_radar_train_fwd_fused(
                C.byref(pv), hs_last.data_ptr(), ref_last.data_ptr(), last_box.data_ptr(), tokens.data_ptr(),
                B, T, int(pad_mult), all_cls.data_ptr(), all_box.data_ptr(), tape.data_ptr(), tape.numel(),
                self.dropout, drop_seed, L.stream_ptr()), 'tc_radar_train_fwd_fused')
        else:
            L.check(lib.tc_radar_train_fwd(
                C.byref(w), hs_last.data_ptr(), ref_last.data_ptr(), last_box.data_ptr(), tokens.data_ptr(),
                B, T, int(pad_mult), all_cls.data_ptr(), all_box.data_ptr(), tape.data_ptr(), tape.numel(),
                self.dropout, drop_seed, L.stream_ptr()), 'tc_radar_train_fwd')
        raw_losses = None
        if self.device_loss:
            from .device_loss import detr_loss_device
            # (a callable is asked for the frames only when a look-ahead is really started: a loader hands over the
            # window that FOLLOWS the frame this iteration trains on)
            # a batched look-ahead (P > 1) is started ONE iteration before the frames in use run out: the batch is
            # ~1.2 ms of device work beside a 1 ms iteration, and the iteration that takes its first frame would wait
            # for all of it (measured: 1.70 instead of 0.96 ms once per batch)
            pend = self.lookahead_pending()
            start = prefetch is not None and self._pre_next is None and \
                pend <= (1 if self.prefetch_depth > 1 else 0)
            hook = (lambda: self.prefetch_decoder(skip=pend, **(prefetch(pend) if callable(prefetch) else prefetch))) \
                if start else None
            if self.chain_backward:      # the non-finite guard of the loss gradients happens inside the backward chain
                losses, d_cls, d_box, _, raw_losses = detr_loss_device(
                    head, all_cls, all_box, gt_bboxes_list, gt_labels_list, before_sync=hook, defer_guard=True)
            else:
                losses, d_cls, d_box, _ = detr_loss_device(head, all_cls, all_box, gt_bboxes_list,
                                                           gt_labels_list, before_sync=hook)
        else:                                              # the reference's PyTorch loss + autograd
            cls_leaf = all_cls.requires_grad_(True)
            box_leaf = all_box.requires_grad_(True)
            outs = {'all_cls_scores': cls_leaf, 'all_bbox_preds': box_leaf,
                    'enc_cls_scores': None, 'enc_bbox_preds': None}
            losses = head.loss(gt_bboxes_list, gt_labels_list, outs)
            total = sum(v for k, v in losses.items() if 'loss' in k)
            total.backward()                               # d loss / d outputs only
            d_cls, d_box = cls_leaf.grad.contiguous(), box_leaf.grad.contiguous()
        self.bucket.zero_grad(check_views=self._gtab_key is None)
        # the gradient pointers are views into the flat bucket: they do not move between iterations
        gkey = self.bucket.grads.data_ptr()
        if self._gtab_key != gkey:
            self._gtab, self._gtab_key = grad_table(head), gkey
        g = self._gtab
        if self.chain_backward:
            bws = self._backward_workspace(lib, w, key, B, T, tokens.device)
            clean = torch.empty_like(raw_losses) if raw_losses is not None else None
            common = (C.byref(w), C.byref(g), hs_last.data_ptr(), last_box.data_ptr(), tokens.data_ptr(), B, T,
                      int(pad_mult), all_box.data_ptr(), d_cls.data_ptr(), d_box.data_ptr(), tape.data_ptr(),
                      tape.numel(), bws.data_ptr(), bws.numel(), self.dropout, drop_seed,
                      raw_losses.data_ptr() if raw_losses is not None else None,
                      clean.data_ptr() if clean is not None else None)
            chunked = self._exchange_in_chunks(update)
            flags = (1 if self._wT_ready else 0) | (2 if chunked else 0)
            common = common + (flags,)
            if self.deterministic:
                need = self.bucket.numel + NF * B * T * 2 * head.embed_dims + 8
                if self._shadow is None or self._shadow.numel() < need or self._shadow.device != tokens.device:
                    self._shadow = torch.zeros(need, dtype=torch.int64, device=tokens.device)   # the call leaves it zero
                L.check(lib.tc_radar_train_bwd_fused_det(*common, self.bucket.grads.data_ptr(), self.bucket.numel,
                                                         self._shadow.data_ptr(), self._shadow.numel(), L.stream_ptr()),
                        'tc_radar_train_bwd_fused_det')
            else:
                L.check(lib.tc_radar_train_bwd_fused_ex(*common, L.stream_ptr()), 'tc_radar_train_bwd_fused_ex')
                if chunked:
                    # the weight gradients chunk by chunk, each chunk's all-reduce started behind its launch: it travels
                    # (RCCL's stream) while the compute stream forms the next chunk
                    chunk_pending = []
                    for gi in range(len(self.bucket.chunk_ranges)):
                        L.check(lib.tc_radar_train_bwd_weights(
                            C.byref(w), C.byref(g), hs_last.data_ptr(), tokens.data_ptr(), B, T, tape.data_ptr(),
                            tape.numel(), bws.data_ptr(), bws.numel(), gi, L.stream_ptr()), 'tc_radar_train_bwd_weights')
                        if self.chunk_events is not None:
                            ev = torch.cuda.Event(enable_timing=True)
                            ev.record()
                            self.chunk_events.append((gi, ev))
                        chunk_pending.append(self.bucket.all_reduce_chunk_begin(gi))
            if clean is not None:
                from .device_loss import loss_dict
                losses = loss_dict(clean)
        else:
            L.check(lib.tc_radar_train_bwd(
                C.byref(w), C.byref(g), hs_last.data_ptr(), last_box.data_ptr(), tokens.data_ptr(), B, T,
                int(pad_mult), all_box.data_ptr(), d_cls.data_ptr(), d_box.data_ptr(), tape.data_ptr(),
                tape.numel(), self.dropout, drop_seed, L.stream_ptr()), 'tc_radar_train_bwd')
        self.last_dropout_seed = drop_seed
        self._sq_clean = True                  # bucket.zero_grad above cleared it and nothing has added to it since
        if self.keep_last:        # tests: the operands of the backward call
            self._last = dict(w=w, g=g, hs_last=hs_last, last_box=last_box, tokens=tokens, B=B, T=T, pad_mult=int(pad_mult),
                              all_box=all_box, d_cls=d_cls, d_box=d_box, tape=tape, seed=drop_seed)
        if update:
            # the gradient exchange starts the moment the backward is enqueued; the optimizer waits on its handle
            # (tools/train.py:253-260: DDP's buckets overlap the same way).  `exchange_events` (bench.py --full --train):
            # how long the compute stream stood still between the backward's end and the optimizer's first kernel
            pending = chunk_pending if (self.chain_backward and chunked) else self.bucket.all_reduce_begin()
            ev = None
            if self.exchange_events is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            self._optimizer_step(lr, pending=pending, mark=ev)
        return {k: v.detach() for k, v in losses.items()}

    def finish(self):
        """Call at the end of an epoch, before an evaluation and before a checkpoint is written (``state_dict`` below does):
        waits for the status words of every iteration still in flight and raises the ValueError scipy raises in the
        reference (ASSIGN:117-125) if one of them met a non-finite cost matrix -- `step_fused_nhwc` polls without a
        synchronisation and would report the LAST iteration only at a next one that never comes."""
        if self.device_loss:
            from .device_loss import check_assign_status
            check_assign_status(self.head, wait=True)

    def state_dict(self):
        """The head's parameters (the reference's keys; they ALIAS the live bucket) + the flat optimizer state in the layout
        of this bucket, without names; `finish()` first.  To write a run out and resume it: ``checkpoint()`` below."""
        self.finish()
        return dict(head=self.head.state_dict(), m=self.m.clone(), v=self.v.clone(), iter=self.iter)

    # ------------------------------------------------------------------
    # checkpoint / resume (transcar_amd/checkpoint.py: the format)
    # ------------------------------------------------------------------
    @staticmethod
    def _world_size():
        return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1

    def _layout(self):
        """(names, shapes, offsets) of the bucket, in the order of ``head.trainable_parameters()``."""
        b = self.bucket
        return b.names, [tuple(p.shape) for p in b.items], b.offsets

    def _bucket_order(self):
        """The parameter names in the order they lie in the bucket."""
        b = self.bucket
        return [b.names[i] for i in sorted(range(len(b.names)), key=lambda i: b.offsets[i])]

    def _adopt_clip_order(self, order):
        """The gradient clip is the one place where an iteration's arithmetic depends on the LAYOUT of the bucket: its
        coefficient comes from a float sum of squares over the bucket in bucket order (tc_sq_norm: fixed workgroup
        partials), and another order rounds differently -- in the last bit of the coefficient, and of every parameter.  A
        run continued from a checkpoint of another layout therefore keeps summing in the order of the run it continues
        (``order``: that run's parameter names as they lay in its bucket): the gradients are gathered into a scratch of
        that layout (one index_select) and tc_sq_norm reads the scratch.  None, or this bucket's own order: nothing."""
        b = self.bucket
        if order is None or list(order) == self._bucket_order():
            self._clip_order = self._clip_index = self._clip_scratch = None
            return
        where = dict(zip(b.names, zip(b.offsets, (p.numel() for p in b.items))))
        index = torch.cat([torch.arange(where[n][0], where[n][0] + where[n][1], dtype=torch.int32) for n in order])
        assert index.numel() == b.numel
        self._clip_order = [str(n) for n in order]
        self._clip_index = index.to(b.grads.device)
        self._clip_scratch = torch.empty_like(b.grads)

    def checkpoint(self, meta=None, to_cpu=True):
        """Everything that decides the next iteration, as one dict ``torch.load(weights_only=True)`` reads back:
        ``state_dict`` (the head's, the reference's keys, CLONED -- ``state_dict()['head']`` above aliases the live bucket),
        ``optimizer`` (the Adam moments per parameter BY NAME, in the form torch.optim.AdamW loads), ``trainer`` (iteration,
        hyper-parameters the optimizer entry does not hold, the dropout seed and the head's forward counter every mask is
        derived from) and ``meta`` (the caller's: epoch, iteration, what ``cosine_lr`` needs).  `finish()` first.
        to_cpu=False leaves the tensors on the device."""
        from . import checkpoint as K
        self.finish()
        names, shapes, offsets = self._layout()
        m, v = (self.m.cpu(), self.v.cpu()) if to_cpu else (self.m, self.v)
        opt = K.pack_optimizer_state(names, shapes, offsets, m, v, self.iter,
                                     dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay))
        head = self.head
        trainer = dict(iter=int(self.iter), seed=int(self.seed), dropout=float(self.dropout),
                       decoder_dropout=float(self.decoder_dropout),
                       max_norm=None if self.max_norm is None else float(self.max_norm),
                       train_forwards=int(head._train_forwards),
                       dropout_seed=int(head.dropout_seed),
                       num_fusion_layers=int(head.num_fusion_layers), deterministic=bool(self.deterministic),
                       prefetch_depth=int(self.prefetch_depth), world_size=int(self._world_size()),
                       # the order the clip's sum of squares runs over the parameters (`_adopt_clip_order`)
                       bucket_order=list(self._clip_order or self._bucket_order()))
        return K.make_checkpoint(head.state_dict(), opt, trainer, meta, to_cpu)

    def load_checkpoint(self, ckpt, strict=True):
        """Continue from ``checkpoint()``'s dict: the head's weights (in place -- the parameters stay views of the bucket
        and a FramePipeline captured on this head keeps replaying), the Adam moments scattered BY NAME into this bucket's
        layout, the iteration, hyper-parameters, dropout seed and forward counter.  With ``deterministic=True`` the
        iterations that follow are bit-identical to those of the run that was not interrupted.
        Also read: a reference-style ``{'meta', 'state_dict', 'optimizer'}`` file (keys under ``pts_bbox_head.``, other
        prefixes ignored; a positional optimizer entry must have this trainer's number of parameters) and the legacy
        ``state_dict()`` dict -- its flat moments carry no names, so all that can be checked is their length: they are
        right only if the bucket that wrote them had this bucket's layout (same ``num_fusion_layers``, same version).
        Refused (TransCARHipError, nothing is changed): another ``num_fusion_layers``, another set of trainable parameters,
        moments of another shape, amsgrad / maximize, steps that differ between parameters.  ``deterministic``,
        ``prefetch_depth`` and the world size stay what the constructor / launcher made them: a difference is reported.
        A checkpoint of another bucket LAYOUT (same names, other offsets) loads like any other; the clip's sum of squares
        then keeps the order of the run that is continued (`_adopt_clip_order`), so that run too continues bit for bit.
        -> dict(form, missing_keys, unexpected_keys, differed={key: (checkpoint's, this trainer's)}, not_restored=[keys],
        clip_sum_order='bucket' | 'checkpoint')."""
        from . import checkpoint as K
        self.finish()
        head, b = self.head, self.bucket
        names, shapes, offsets = self._layout()
        report = dict(form='named', missing_keys=[], unexpected_keys=[], differed={}, not_restored=[])
        m_new, v_new = torch.empty_like(self.m), torch.empty_like(self.v)
        if K.is_legacy(ckpt):
            report['form'] = 'legacy'
            if ckpt['m'].numel() != b.numel or ckpt['v'].numel() != b.numel:
                raise L.TransCARHipError('legacy checkpoint: %d moments for a bucket of %d elements'
                                         % (ckpt['m'].numel(), b.numel))
            sd = K.clone_tensors(K.head_state_dict(ckpt['head']))     # (its tensors may alias this very bucket)
            missing = [n for n in names if n not in sd]
            if missing:
                raise L.TransCARHipError('legacy checkpoint lacks trainable parameter(s) %s' % K._some(missing))
            m_new.copy_(ckpt['m'].reshape(-1))
            v_new.copy_(ckpt['v'].reshape(-1))
            step, hyper, saved = int(ckpt['iter']), None, {}
            report['not_restored'] = ['lr', 'betas', 'eps', 'weight_decay'] + [k for k in K.RESTORED if k != 'iter']
        else:
            sd = K.check_structure(ckpt, names, head.num_fusion_layers)
            opt, saved = ckpt.get('optimizer'), dict(ckpt.get('trainer') or {})
            if opt is None:
                report['form'], step, hyper = 'weights', None, None
                report['not_restored'] = ['optimizer']
            else:
                if opt.get('param_names') is None:
                    report['form'] = 'positional'
                step = K.unpack_optimizer_state(opt, names, shapes, offsets, m_new, v_new)
                hyper = K.optimizer_hyper(opt)
            if 'iter' in saved and step is not None and int(saved['iter']) != step:
                raise L.TransCARHipError('checkpoint: trainer iteration %d, optimizer step %d' % (int(saved['iter']), step))
            report['not_restored'] += [k for k in K.RESTORED if k not in saved and not (k == 'iter' and step is not None)]
            if saved.get('bucket_order') is not None and sorted(saved['bucket_order']) != sorted(names):
                raise L.TransCARHipError('checkpoint: bucket_order does not hold the trainable parameters once each')
        own = head.state_dict()
        bad = ['%s %s (the head: %s)' % (k, tuple(t.shape), tuple(own[k].shape)) for k, t in sd.items()
               if k in own and tuple(t.shape) != tuple(own[k].shape)]
        if strict:
            bad = ['%s (missing)' % k for k in own if k not in sd] + ['%s (unexpected)' % k for k in sd if k not in own] + bad
        if bad:
            raise L.TransCARHipError('checkpoint state_dict does not fit the head: %s' % K._some(bad))
        # -- nothing was changed so far, and nothing is refused from here on
        if head.query_embedding.weight.is_cuda:
            torch.cuda.synchronize(head.query_embedding.weight.device)    # replays / iterations in flight read the old values
        res = head.reload_state_dict(sd, strict=strict)
        report['missing_keys'], report['unexpected_keys'] = list(res.missing_keys), list(res.unexpected_keys)
        if step is not None:
            self.m.copy_(m_new)
            self.v.copy_(v_new)
            self.iter = int(step)
            self._adopt_clip_order(saved.get('bucket_order'))
            report['clip_sum_order'] = 'bucket' if self._clip_index is None else 'checkpoint'
        if hyper is not None:
            self.lr, self.betas, self.eps = hyper['lr'], hyper['betas'], hyper['eps']
            self.weight_decay = hyper['weight_decay']
        if 'seed' in saved:
            self.seed = int(saved['seed'])
        if 'dropout' in saved:
            self.dropout = float(saved['dropout'])
        if 'decoder_dropout' in saved:
            self.decoder_dropout = float(saved['decoder_dropout'])
        if 'max_norm' in saved:
            self.max_norm = None if saved['max_norm'] is None else float(saved['max_norm'])
        if 'dropout_seed' in saved:
            head.dropout_seed = int(saved['dropout_seed'])
        if 'train_forwards' in saved:
            head._train_forwards = int(saved['train_forwards'])
        mine = dict(deterministic=bool(self.deterministic), prefetch_depth=int(self.prefetch_depth),
                    world_size=int(self._world_size()))
        for k in K.COMPARED:
            if k in saved and saved[k] != mine[k]:
                report['differed'][k] = (saved[k], mine[k])
        self.invalidate_lookahead()           # a pending look-ahead drew the masks of the old counter from the old weights
        self._sq_clean = False
        return report

    def save_checkpoint(self, path, meta=None):
        """``checkpoint(meta)`` to ``path``, atomically (written beside it, then renamed).  With a process group rank 0
        writes and every rank waits for the file."""
        import os
        ckpt = self.checkpoint(meta)           # (every rank: finish() is this rank's own)
        grouped = dist.is_available() and dist.is_initialized()
        if not grouped or dist.get_rank() == 0:
            tmp = str(path) + '.tmp'
            torch.save(ckpt, tmp)
            os.replace(tmp, str(path))
        if grouped:
            dist.barrier()

    def load_checkpoint_file(self, path, map_location=None, strict=True):
        """``load_checkpoint`` of a file ``save_checkpoint`` (or mmcv) wrote.  Every rank loads the same file: the
        parameters agree, the dropout masks differ by rank as before (Detr3DHead.next_dropout_seed)."""
        return self.load_checkpoint(torch.load(str(path), map_location=map_location, weights_only=True), strict=strict)

    def _exchange_in_chunks(self, update=True):
        """Chunked weight-gradient launches + one all-reduce per chunk: only where there is an exchange to hide (more than
        one rank), on the fused float-atomic backward, and only with the N + 1 chunks the C entry knows (N fusion layers)."""
        return bool(update and self.chunked_exchange and self.chain_backward and not self.deterministic
                    and len(self.bucket.chunk_ranges) == self.head.num_fusion_layers + 1
                    and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)

    def _backward_workspace(self, lib, w, key, B, T, device):
        if self._bws_key != key:
            self._bws = L.device_bytes(device, lib.tc_radar_train_bwd_workspace_bytes, C.byref(w), B, T)
            self._bws_key = key
        return self._bws

    def _optimizer_step(self, lr=None, pending=None, mark=None):
        if mark is not None and isinstance(pending, list):
            # (bench.py --full --train: how long the compute stream waits for EACH chunk's all-reduce, in the order it waits)
            evs, world = [mark[0]], 1
            for work, wld in pending:
                if work is not None:
                    work.wait()
                world = wld
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                evs.append(e)
            if self.exchange_chunk_events is not None:
                self.exchange_chunk_events.append(evs)
        else:
            world = self.bucket.all_reduce_end(pending) if pending is not None else self.bucket.all_reduce()
        if mark is not None:
            mark[1].record()
            self.exchange_events.append(mark)
        b, lib = self.bucket, L.lib()
        self.iter += 1
        if not self._sq_clean:                 # (zeroed with the gradients in the fused iteration)
            self.sq.zero_()
        self._sq_clean = False
        grads = b.grads
        if self._clip_index is not None:       # a run continued from another bucket layout: its order of the float sum
            grads = torch.index_select(b.grads, 0, self._clip_index, out=self._clip_scratch)
        L.check(lib.tc_sq_norm(grads.data_ptr(), b.numel, self.sq.data_ptr(), L.stream_ptr()),
                'tc_sq_norm')
        L.check(lib.tc_adamw_step(
            b.params.data_ptr(), b.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), b.numel,
            float(self.lr if lr is None else lr), self.betas[0], self.betas[1], self.eps,
            self.weight_decay, self.iter, 1.0 / world, float(self.max_norm or 0.0),
            self.sq.data_ptr(), L.stream_ptr()), 'tc_adamw_step')
        self.head.mark_trainable_dirty()      # re-packed lazily by the next inference forward / replay

    def step(self, mlvl_feats, img_metas, gt_bboxes_list, gt_labels_list, lr=None):
        """One iteration on this rank's frame(s); returns the loss dict (detached)."""
        self.head.train()
        outs = self.head(mlvl_feats, img_metas)
        losses = self.head.loss(gt_bboxes_list, gt_labels_list, outs)
        self.backward_and_step(losses, lr)
        return {k: v.detach() for k, v in losses.items()}

    def step_nhwc(self, feats_nhwc, lidar2img, img_hw, tokens, pad_mult, gt_bboxes_list,
                  gt_labels_list, lr=None):
        """Same with everything already resident on the device (bench)."""
        self.head.train()
        outs = self.head.forward_train_nhwc(feats_nhwc, lidar2img, img_hw, tokens, pad_mult)
        losses = self.head.loss(gt_bboxes_list, gt_labels_list, outs)
        self.backward_and_step(losses, lr)
        return {k: v.detach() for k, v in losses.items()}
