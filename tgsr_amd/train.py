"""SR generator training step (the loop the reference never shipped - SURVEY section 3.3).

What the reference pins down and this harness uses: the loss functions and their conventions (`MSE` losses.py:779,
`KL_loss` :806, `generator_loss` / `discriminator_loss` :290-391 when a discriminator is supplied), labels
(`prepare_labels`, trainer_objective.py:43-53), Adam(lr 2e-4, betas (0.5, 0.999)) (config.py:37-38,
pretrain_DAMSM.py:270), the EMA helpers `copy_G_params` / `load_params` (miscc/utils.py:467-474), BatchNorm in
training mode.  What it does NOT pin down (no caller exists): loss weights, update order, the discriminator
architecture (no class anywhere in the reference) and the Inception image encoder (third-party weights).  This
harness therefore trains the two generators on the pixel + KL terms,
    errG = MSE(fake_imgL, HR pyramid) + MSE(fine_im, HR pyramid) + KL(mu, logvar),
and takes the adversarial / DAMSM terms only when the caller supplies `netsD` / `image_encoder` (the DAMSM term
`words_loss + sent_loss` on `image_encoder(fine_im[-1])` is differentiable through the HIP DAMSM backward kernel).
Every forward and backward kernel of the generators is HIP (tgsr_amd.autograd); the text encoder is frozen (eval).
`DAMSMTrainer` is the counterpart of pretrain_DAMSM.py (text encoder + CNN_ENCODER heads on the matching losses).
Data parallel: gradients live in one flat bucket, one all-reduce per step (tgsr_amd.parallel.FlatGradBucket).
"""
import contextlib
import os
import statistics
import time
import warnings

import numpy as np
import torch
import torch.distributed as dist

from . import autograd, featdist, lpips as lpips_mod, metrics, model, niqe as niqe_mod, parallel, retrieval
from .miscc import losses
from .miscc.config import cfg
from .miscc.utils import copy_G_params, load_params  # noqa: F401  (miscc/utils.py:467-474: the generator EMA helpers)
from .model import CNN_ENCODER, G_SR_NET_low, NetG_highweight, RNN_ENCODER
from .optim import FlatAdam
from .parallel import FlatGradBucket, RcclDirect, dp_world
from .trainer import SRPipeline, caption_mask, distinct_streams


def prepare_labels(batch_size, device):
    """trainer_objective.py:43-53."""
    return (torch.ones(batch_size, device=device), torch.zeros(batch_size, device=device),
            torch.arange(batch_size, device=device))


def snapshot_due(epoch, max_epoch=None):
    """The snapshot rule of the reference's training loops (pretrain_DAMSM.py:286-287)."""
    max_epoch = cfg.TRAIN.MAX_EPOCH if max_epoch is None else max_epoch
    return epoch % cfg.TRAIN.SNAPSHOT_INTERVAL == 0 or epoch == max_epoch


# eager G/D steps before the discriminator updates are captured (allocator, streams and Adam state warm)
GRAPH_D_WARMUP = 3
# eager steps before the generators' update is captured (the same, plus every weight pack of the step in the PackCache)
GRAPH_G_WARMUP = 3
# TGSR_GRAPH_G=auto: steps of each form (eager, replayed) the trainer times before it settles on the faster one
GRAPH_G_TRIALS = 3
# ... and the number of steps after which that choice has been made (warm-up, eager trials, the capturing step, replayed trials)
GRAPH_G_SETTLED = GRAPH_G_WARMUP + 2 * GRAPH_G_TRIALS + 1


class GraphPolicy:
    """Which form the generators' update takes - eager or replayed from hipGraphs - and, for TGSR_GRAPH_G=auto, the measurement that
    decides it.  `graph` is the form in force (the first guess until measured, then the faster one, or whatever `pin` was given);
    while `measuring`, step k's form is a function of k alone: steps [WARMUP, WARMUP + TRIALS) are timed eager, step
    WARMUP + TRIALS captures (untimed), the next TRIALS are timed replays, and the end of step GRAPH_G_SETTLED - 1 decides by the
    medians.  The owner supplies `clock()` (seconds, the device idle) and `reduce_max(te, tp)` (the slowest rank's times, so that
    every rank takes the same form).  `report` is what the trainer publishes as `graph_policy`."""

    def __init__(self, mode, prior, measuring, clock=time.perf_counter, reduce_max=lambda te, tp: (te, tp)):
        self.mode, self.graph, self.measuring = mode, bool(prior), bool(measuring)
        self.clock, self.reduce_max = clock, reduce_max
        self.eager_s, self.replay_s, self.t0, self.form = [], [], None, None
        self.report = {"mode": mode, "prior": "replay" if prior else "eager"}

    def pin(self, graph):
        """An explicit choice: it ends the measurement."""
        self.graph, self.measuring = bool(graph), False

    def replays(self, k):
        """Does step k take the replayed form (once the warm-up is over)?"""
        return (self.form == "replay" if self.measuring else self.graph) and k >= GRAPH_G_WARMUP

    def begin(self, k):
        """The top of step k: its form while the policy is measuring, and the start of its clock if it is a timed one."""
        if not self.measuring:
            return
        self.form = "eager" if k < GRAPH_G_WARMUP + GRAPH_G_TRIALS else "replay"
        timed = GRAPH_G_WARMUP <= k and k != GRAPH_G_WARMUP + GRAPH_G_TRIALS
        self.t0 = self.clock() if timed else None

    def end(self, k, replayed):
        """The end of step k (`replayed`: it really ran from the graphs); the last measured step decides."""
        if not self.measuring:
            return
        if self.t0 is not None:
            dt = self.clock() - self.t0
            if self.form == "replay":
                self.replay_s.append(dt if replayed else float("inf"))     # (the capture failed or the configuration has none)
            else:
                self.eager_s.append(dt)
        if k + 1 < GRAPH_G_SETTLED:
            return
        inf = float("inf")
        te = statistics.median(self.eager_s) if self.eager_s else inf      # (steps that raised may have left a form untimed)
        tp = statistics.median(self.replay_s) if self.replay_s else inf
        te, tp = self.reduce_max(te, tp)
        if te == inf:                                               # nothing to compare with: the first guess stands
            self.pin(self.graph)
            self.report["chosen"] = "replay" if self.graph else "eager"
            return
        self.pin(tp <= te)
        self.report.update({"eager_ms": round(te * 1e3, 3), "replay_ms": None if tp == inf else round(tp * 1e3, 3),
                            "chosen": "replay" if tp <= te else "eager",
                            "trials": "median of %d steps of each form, device idle on both sides" % GRAPH_G_TRIALS})


class SRTrainer:
    def __init__(self, n_words, device="cuda", low="lr", lr=None, ema_decay=0.999, image_encoder=None,
                 discriminators=False, d_lr=None, gather_negatives=None, weightmap=False, use_act=True, pixel_loss="mse",
                 reweight=False, cycle=0.0, perceptual=None):
        """image_encoder: optional frozen module image [B,3,256,256] -> (region features [B,nef,17,17], cnn_code
        [B,nef]) (a CNN_ENCODER with its trunk): adds the DAMSM ranking term of generator_loss (losses.py:375-386)
        on the finest image, x TRAIN.SMOOTH.LAMBDA.
        discriminators: True builds one discriminator per output scale (model.D_NET64 / 128 / 256 for the x8
        generators' 64 / 128 / 256 images) or pass a list of modules exposing COND_DNET / UNCOND_DNET; `step()` then
        alternates the discriminator update (discriminator_loss, losses.py:290-316) and the generator update
        (generator_loss :351-391 + MSE + KL), each discriminator with its own Adam(DISCRIMINATOR_LR, betas (0.5, 0.999))
        and flat gradient bucket.  The reference defines the two loss functions but neither the discriminators nor the
        loop: architecture and update order (D first, then G on the same fake images, as in the AttnGAN
        trainer TGSR was forked from) are the build's declaration.
        weightmap / use_act: NetG_highweight's form (model.py:212-298).  weightmap=True trains the maps a1..a3 (64 / 128 /
        256 pixels: 32 x 32 LR) with the other generator parameters (flat gradient bucket, Adam, EMA); use_act=False drops
        the heads' Tanh.
        pixel_loss: "mse" (default) or "weight_mse" - the pixel term becomes weight_MSE(fake_imgL, HR, att)[0] + weight_MSE(fine_im,
        HR, att)[0] (losses.py:792-804) on the three attention maps G_SR_NET_low returns (32^2 / 64^2 / 128^2 under the 64^2 / 128^2 /
        256^2 images).  The reference ships no training loop: pairing both generators' images with the same maps is the build's
        declaration, like the update order.  The maps leave the generator's attention kernels without a gradient path, so the term
        reads them as weights.
        reweight: the ranking term scales every word by the confidence of the LAST attention map (words_reweight_loss /
        generator_re_weight_loss, losses.py:137-232, 318-350; detached, as there); needs `image_encoder`.
        Either option keeps the generators' update on the eager path (`_g_graphs`); reweight with gather_negatives and more than
        one rank is refused: the confidences would have to be gathered with the words.
        cycle: weight of the cycle-consistency term (default 0.0: the term does not exist).  With cycle > 0 the generators' loss gains
        cycle * (CycleMSE(fake_imgL, LR) + CycleMSE(fine_im, LR)) (losses.py:785-790): both generators' pyramids, resized back to
        the LR size by bicubic interpolation, are held to `LR`, the step's own LR input.  The reference defines the function and ships
        no training loop: which images it is applied to, and against which LR tensor, is the build's declaration, like the pairing
        above.  Each call is one forward and one backward launch of tgsr_cycle_mse.hip with nothing on the host that depends on
        data, so - unlike the attention-guided options - the term leaves the generators' update on the captured path.  It is a
        per-shard batch mean like MSE: nothing to do for data parallelism.
        perceptual: None (default: the term does not exist and the trainer is what it is without the argument) or (model, weight), a
        tgsr_amd.lpips.LPIPS (or the path of a saved one) and a finite weight >= 0.  The generators' loss gains
        weight * mean_b LPIPS(fine_im[-1], HR[-1]): the raw float output of the finest scale against its ground truth, one term.  The
        reference has no such term: this is the build's declaration.  The walk (trunk forward, tails, the tape in reverse) holds
        nothing on the host that depends on data, so the term leaves the generators' update on the captured path; the filters are
        packed here, before any capture.  A per-shard batch mean like MSE.  A meaningful term needs trained LPIPS weights, which are
        not shipped."""
        self.perceptual, self.perceptual_weight = None, 0.0
        if perceptual is not None:
            if not isinstance(perceptual, (tuple, list)) or len(perceptual) != 2:
                raise ValueError("perceptual must be None or (an LPIPS model, a weight), got %r" % (perceptual,))
            try:
                self.perceptual_weight = float(perceptual[1])
            except (TypeError, ValueError):
                self.perceptual_weight = float("nan")
            if not self.perceptual_weight >= 0.0 or self.perceptual_weight == float("inf"):
                raise ValueError("perceptual: the weight must be finite and >= 0, got %r" % (perceptual[1],))
            self.perceptual = lpips_mod.as_model(perceptual[0], device, "perceptual: the model")
            if torch.device(device).type == "cuda":
                with torch.cuda.device(torch.device(device)):
                    self.perceptual.refresh()
        self.cycle = float(cycle)
        if not self.cycle >= 0.0 or self.cycle == float("inf"):
            raise ValueError("cycle must be a finite weight >= 0, got %r" % (cycle,))
        self._lr_in, self.cycle_fused = None, None     # the step's LR input (kept only with cycle > 0); `fused` of CycleMSE
        if pixel_loss not in ("mse", "weight_mse"):
            raise ValueError("pixel_loss must be 'mse' or 'weight_mse', got %r" % (pixel_loss,))
        self.pixel_loss, self.reweight = pixel_loss, bool(reweight)
        if self.reweight and image_encoder is None:
            raise ValueError("reweight=True re-weights the DAMSM ranking term: it needs an image_encoder")
        self._att, self.attn_fused = None, None        # the step's attention maps; `fused` of the attention-guided losses
        self.device = torch.device(device)
        cuda = self.device.type == "cuda"
        # data parallel: the DAMSM ranking term on the gathered global batch (parallel.GATHER_NEGATIVES, default on) or per shard
        self.gather_negatives = parallel.GATHER_NEGATIVES if gather_negatives is None else bool(gather_negatives)
        self._check_reweight()
        self._packs = autograd.PackCache() if (cuda and os.environ.get("TGSR_PACK_CACHE", "1") != "0") else None
        self.image_encoder = image_encoder
        self.text_encoder = RNN_ENCODER(n_words, nhidden=cfg.TEXT.EMBEDDING_DIM).to(self.device).eval()
        for p in self.text_encoder.parameters():
            p.requires_grad = False
        self.netGL = G_SR_NET_low().to(self.device).train()
        self.netGH = NetG_highweight(weightmap=bool(weightmap), low=low, useAct=bool(use_act)).to(self.device).train()
        self.params = list(self.netGL.parameters()) + list(self.netGH.parameters())
        # (BatchNorm's running statistics ride the gradient bucket's all-reduce: identical on every rank, parallel.py.)
        # Bucket layout [NetG_highweight | G_SR_NET_low | buffers]: backward runs through NetG_highweight first (its nodes
        # are the younger ones), so its gradients are final while G_SR_NET_low's backward still runs - that range goes out
        # early (`_fire_early`), the rest with the step's closing all-reduce: two collectives, the first under backward.
        gh_params = [p for p in self.netGH.parameters() if p.requires_grad]
        self._bucket_bufs = list(self.netGL.buffers()) + list(self.netGH.buffers())
        self._gh_params = gh_params
        self._early_n = len(gh_params)                                   # parameters of the early range
        self._early_hi = None                                            # ... = flat[0:_early_hi], set once the bucket exists
        self._early_on = os.environ.get("TGSR_EARLY_ALLREDUCE", "1") != "0"
        self._early_left, self._early = -1, None
        for p in gh_params:
            p.register_post_accumulate_grad_hook(self._gh_grad_done)
        self._fused_adam = cuda and os.environ.get("TGSR_FUSED_ADAM", "1") != "0"
        # The generators' update - forward, losses, backward, Adam, re-pack, EMA - holds no host decision once the text encoder has
        # produced the embeddings: it is replayed from hipGraphs (one per batch shape), in segments with the gradient all-reduce
        # BETWEEN them, so the replayed step also exists with more than one rank (`_capture_g`).  TGSR_GRAPH_G=0: eager.
        # Default ("auto"): replay where it measured at least as fast as the eager step on an idle host - the G/D alternation
        # (20.6 vs 20.9 ms); the generator-only step (10.0-10.3 vs 9.9 ms) and the step with the Inception encoder (38.8 vs 35.2 ms:
        # ~1 000 more small kernels, each dependent node of a replay costs a few microseconds more than a launch from a host that
        # keeps ahead) stay eager: the steps are DEVICE-bound (kernel time 12.1 ms, busy 9.6 ms of a 9.9 ms generator step), so
        # taking the host out buys nothing there.  TGSR_GRAPH_G=1 replays all of them (a loaded or slower host: under rocprofv3
        # the replayed generator step runs 10.7 ms, the eager one 15.7), 0 none.
        # Which of the two wins is a property of the HOST the process lands on (round 6: the same tree ran the eager generator
        # step in 9.9 ms on one box and 12.0 ms on another, whose replays would have taken 10.3), so "auto" MEASURES: after the
        # warm-up it times GRAPH_G_TRIALS eager steps, captures, times as many replayed ones and keeps the faster form (with
        # several ranks: the slowest rank's times, so that every rank takes the same one).  The rule above is only the form the
        # first steps take; assigning `_graph_g` by hand ends the measurement and pins the form.
        mode = os.environ.get("TGSR_GRAPH_G", "auto")
        self._graph_capable = cuda and mode != "0"
        self._policy = GraphPolicy(mode, prior=cuda and (mode == "1" or (mode == "auto" and bool(discriminators) and image_encoder is None)),
                                   measuring=cuda and mode == "auto", clock=self._idle_clock, reduce_max=self._max_over_ranks)
        self._ggraphs, self._gsteps, self._ghyper = {}, 0, None
        # TGSR_FLAT_ADAM (default on, HIP only): parameters and moments re-homed into flat buffers beside the flat gradient bucket,
        # the update ONE launch of tgsr::adam_flat_ (optim.FlatAdam; the same rule as torch.optim.Adam); 0 = torch's fused Adam
        self._flat_adam = cuda and os.environ.get("TGSR_FLAT_ADAM", "1") != "0"
        self._g_lr = lr or cfg.TRAIN.GENERATOR_LR
        self.ema_decay = ema_decay
        self.avg_param_G = copy_G_params(self.netGL) + copy_G_params(self.netGH)
        self.netsD, self.optsD, self.bucketsD = [], [], []
        self._graph_d, self._dgraphs, self._dsteps, self._d_bump = False, [], 0, []
        if discriminators:
            self.netsD = list(discriminators) if not isinstance(discriminators, bool) else \
                [model.D_NET64(), model.D_NET128(), model.D_NET256()]
            # A discriminator's update - forward on (real, fake.detach()), loss, backward, Adam - is a closed piece of device work
            # with no host decision in it: replayed from a hipGraph per discriminator once the step has run `GRAPH_D_WARMUP` times
            # (with more than one rank as two graphs around the bucket's all-reduce: `_capture_update`).  ~1 000 of a step's ~1 570
            # launches leave the host that way; the step was issued no faster than 21-25 ms (profiles/HISTORY.md 3.18).  TGSR_GRAPH_D=0: eager.
            self._graph_d = cuda and os.environ.get("TGSR_GRAPH_D", "1") != "0"
            self._dgraphs = [None] * len(self.netsD)
            for d in self.netsD:
                d.to(self.device).train()
                self.bucketsD.append(FlatGradBucket(d.parameters(), buffers=d.buffers()).attach())
                # (fused: one pass over a discriminator's ~70 M parameters and their moments instead of the ~10 of the
                # multi-tensor form - 2.0 ms of a G/D step were Adam kernels running alone on the device)
                self.optsD.append(self._adam(self.bucketsD[-1], d.parameters(), d_lr or cfg.TRAIN.DISCRIMINATOR_LR, self._graph_d))
                self._d_bump.append(list(self.bucketsD[-1].params) + list(d.buffers()))
            # the generator loss runs the train-mode discriminators on the fake images once more (g_loss): their running
            # statistics move again, per rank, AFTER their own bucket's all-reduce - so they also ride the generators' bucket
            # and every rank leaves the step with the same discriminator buffers (a snapshot is the same file on every rank)
            self._bucket_bufs = self._bucket_bufs + [b for d in self.netsD for b in d.buffers()]
        self.bucket = FlatGradBucket(gh_params + list(self.netGL.parameters()), buffers=self._bucket_bufs).attach()
        self._early_hi = self.bucket.offsets[self._early_n][0] if self._early_n < len(self.bucket.params) else self.bucket.numel
        self.opt = self._adam(self.bucket, self.params, self._g_lr, self._graph_capable)
        # what a replayed (or fused-Adam) update writes without telling autograd's version counters (`_bump`)
        self._g_bump = list(self.params) + list(self._bucket_bufs)
        # TGSR_COMM=direct: the buckets' closing all-reduce through the library's own RCCL communicator (tgsr_allreduce_flat,
        # parallel.RcclDirect) instead of torch.distributed's; the early range and the DAMSM gather stay on the process group
        self._rccl = None
        if os.environ.get("TGSR_COMM", "") == "direct" and cuda and dp_world() > 1:
            self._rccl = RcclDirect.create()
            self._early_on = False
            for b in [self.bucket] + self.bucketsD:
                b.comm = self._rccl
        # Every stream of the trainer, each distinct from the current one and from all handed out before it
        # (distinct_streams: torch hands out pool streams round robin - two "new" streams can be the same hip stream)
        taken = [torch.cuda.current_stream(self.device).cuda_stream] if cuda else []

        def streams(n):
            out = distinct_streams(n, self.device, avoid=taken)
            taken.extend(st.cuda_stream for st in out)
            return out
        # the generators' weight gradients run on a side stream beside the data-gradient chain while a step's backward
        # is in flight (12.7 -> 11.7 ms per step at B=16: the small layers' weight-gradient kernels and the slab sums
        # fill a fraction of the CUs); TGSR_WGRAD_SIDE=0 keeps everything on one stream
        self._wside = streams(1)[0] if cuda and os.environ.get("TGSR_WGRAD_SIDE", "1") != "0" else None
        self._comm = streams(1)[0] if cuda else None                     # the early all-reduce (`_fire_early`)
        self._dstreams = streams(len(self.netsD)) if cuda and self.netsD and os.environ.get("TGSR_D_STREAMS", "1") != "0" else []
        # TGSR_D_WGRAD_SIDE=1 (opt-in): each discriminator's weight gradients on a side stream of its own, beside its data-gradient
        # chain - the 256^2 discriminator's update is the longest dependent chain of a G/D step and a quarter of its backward
        # kernels are weight gradients nothing waits for until Adam.  Built, bit-identical (the gan / dp suites pass with it), and
        # SLOWER on this chip: 20.8 against 19.6 ms per G/D step, 31.9 against 30.3 with the ranking term (same box) - the three
        # updates already run side by side, and six streams compete for four hardware queues (GPU_MAX_HW_QUEUES=8 is worse
        # still: 43.6 ms).  Left off.
        self._dwside = streams(len(self._dstreams)) if self._dstreams and os.environ.get("TGSR_D_WGRAD_SIDE", "0") == "1" else []
        # TGSR_ENC_EARLY=1 (opt-in): generator_loss's image encoder (CNN_ENCODER: ~190 launches of small GEMMs forward) reads the fake
        # image only - not the discriminators - so it can be issued BEFORE the discriminator updates, on a stream of its own (as a
        # hipGraph of its own when the step is replayed), and run beside them; its backward stays where it was.  Built, parity-green
        # (the early forms, eager and replayed, are bit-identical; against the late form the fake image's gradient adds its terms in
        # another order) and NOT faster: 29.6 / 29.8 against 28.7 / 29.6 ms (two pairs, one box) - "one kernel in flight" during the
        # 256^2 discriminator's update does not mean idle CUs: its GEMMs fill the chip, and the encoder's kernels only lengthen them.
        self._encst = streams(1)[0] if (cuda and image_encoder is not None and self.netsD and
                                        os.environ.get("TGSR_ENC_EARLY", "0") == "1") else None
        # the stream the generators' graphs are captured on, and the branch their re-pack launches fork onto
        self._gcap, self._gpack = streams(2) if self._graph_capable else (None, None)

    @property
    def _attn_losses(self):
        """A loss of this trainer reads the generator's attention maps (pixel_loss="weight_mse" or reweight)."""
        return self.pixel_loss == "weight_mse" or self.reweight

    def _check_reweight(self):
        if self.reweight and self.gather_negatives and dp_world() > 1:
            raise ValueError("reweight=True with gather_negatives on %d ranks: the ranking term of the gathered global batch would "
                             "need every rank's word confidences gathered too, which is not built; pass gather_negatives=False"
                             % dp_world())

    def _adam(self, bucket, params, lr, capturable):
        """FlatAdam over this bucket (TGSR_FLAT_ADAM), else torch's Adam over `params`: Adam(lr, betas (0.5, 0.999)) either way."""
        if self._flat_adam:
            return FlatAdam(bucket.params, bucket.flat, lr=lr, betas=(0.5, 0.999))
        return torch.optim.Adam(params, lr=lr, betas=(0.5, 0.999), capturable=capturable, fused=self._fused_adam)

    # ------------------------------------------------------------------ TGSR_GRAPH_G: the form of the generators' update (GraphPolicy)
    @property
    def _graph_g(self):
        return self._policy.graph

    @_graph_g.setter
    def _graph_g(self, v):
        self._policy.pin(v)                  # an explicit choice ends the measured policy

    @property
    def _auto(self):
        """The policy while it is still measuring, None once it has settled or was pinned."""
        return self._policy if self._policy.measuring else None

    @property
    def graph_policy(self):
        return self._policy.report

    def _idle_clock(self):
        torch.cuda.synchronize(self.device)
        return time.perf_counter()

    def _max_over_ranks(self, te, tp):
        if dp_world() > 1:
            t = torch.tensor([te, tp], dtype=torch.float64, device=self.device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            te, tp = float(t[0]), float(t[1])
        return te, tp

    # ------------------------------------------------------------------ gradient all-reduce under the tail of backward
    def _arm_early(self):
        self._early = None
        self._early_left = self._early_n if (self._early_on and dp_world() > 1 and self._comm is not None) else -1

    def _gh_grad_done(self, _p):
        """post-accumulate hook of every NetG_highweight parameter: when the last one has its gradient, that range of the
        bucket is final - flush it and start its all-reduce on the communication stream while G_SR_NET_low's backward goes on."""
        if self._early_left <= 0:
            return
        self._early_left -= 1
        if self._early_left == 0:
            self._fire_early()

    def _fire_early(self):
        cur = torch.cuda.current_stream(self.device)
        self.bucket.flush_params(0, self._early_n)
        self._comm.wait_stream(cur)
        if self._wside is not None:
            self._comm.wait_stream(self._wside)            # the weight-gradient kernels of this range run there
        with torch.cuda.stream(self._comm):
            self._early = self.bucket.all_reduce_range_async(0, self._early_hi)

    def _all_reduce(self):
        """The step's closing collective: everything the early one did not take (all of it when none was started)."""
        if self._early is None:
            self._early_left = -1
            self.bucket.all_reduce_mean()
            return
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self._comm):
            self._early.wait()
        cur.wait_stream(self._comm)
        self._early, self._early_left = None, -1
        self.bucket.all_reduce_mean(skip=(0, self._early_hi))

    def loss(self, captions, cap_lens, LR, LRb, hr_pyramid, class_ids=None):
        """hr_pyramid: the 3 target scales [B,3,2s,2s], [B,3,4s,4s], [B,3,8s,8s]."""
        fake_imgL, fine_im, mu, logvar, words_embs, sent_emb = self.forward_G(captions, cap_lens, LR, LRb)
        errG = self._loss_from(fake_imgL, fine_im, mu, logvar, words_embs, sent_emb, cap_lens, hr_pyramid, class_ids)
        return errG, fake_imgL, fine_im

    @staticmethod
    def _zero(bucket):
        """Open a step: one memset of the flat bucket; `.grad` cleared and the gradient slots opened, so the weight-
        gradient kernels write straight into the bucket (parallel.grad_slot) instead of autograd adding into views."""
        bucket.begin_step()

    def _text(self, captions, cap_lens):
        """The frozen text encoder and the caption mask: the only part of a step that reads host data (the caption lengths)."""
        with torch.no_grad():
            words_embs, sent_emb = self.text_encoder(captions, cap_lens, self.text_encoder.init_hidden(captions.shape[0]))
        return words_embs, sent_emb, caption_mask(captions, words_embs.size(2))

    def _forward_nets(self, LR, LRb, words_embs, sent_emb, mask):
        # (NetG_highweight's trunk on a second stream beside G_SR_NET_low, forward and backward, was measured: 11.9 ms
        # against 11.6 ms on one stream once the weight gradients have their side stream - not kept)
        fake_imgL, att, mu, logvar = self.netGL(LR, sent_emb, words_embs, mask)
        self._att = [a.detach() for a in att] if self._attn_losses else None
        self._lr_in = LR if self.cycle > 0 else None
        fine_im, _a, _one = self.netGH(LR, fake_imgL, LRb)
        return fake_imgL, fine_im, mu, logvar

    def forward_G(self, captions, cap_lens, LR, LRb):
        """Text encoder (frozen) + both generators in training mode: (fake_imgL, fine_im, mu, logvar, words, sent)."""
        words_embs, sent_emb, mask = self._text(captions, cap_lens)
        fake_imgL, fine_im, mu, logvar = self._forward_nets(LR, LRb, words_embs, sent_emb, mask)
        return fake_imgL, fine_im, mu, logvar, words_embs, sent_emb

    def d_losses(self, fine_im, hr_pyramid, sent_emb):
        """discriminator_loss (losses.py:290-316) of every scale: real = HR pyramid, fake = the generators' output."""
        B = sent_emb.shape[0]
        real_labels, fake_labels, _ = prepare_labels(B, self.device)
        return [losses.discriminator_loss(d, hr_pyramid[i], fine_im[i], sent_emb, real_labels, fake_labels)
                for i, d in enumerate(self.netsD)]

    def g_loss(self, fake_imgL, fine_im, mu, logvar, words_embs, sent_emb, cap_lens, hr_pyramid, class_ids=None, enc_out=None):
        """generator_loss (losses.py:351-391) on the fine images + the pixel and KL terms of `loss`.  enc_out: the image encoder's
        outputs on the finest fake image when `_encode_early` has computed them already."""
        B = sent_emb.shape[0]
        real_labels, _fake, match_labels = prepare_labels(B, self.device)
        if self.reweight:
            self._check_reweight()
            adv, _log = losses.generator_re_weight_loss(self.netsD, self.image_encoder, fine_im, real_labels, words_embs, sent_emb,
                                                        match_labels, cap_lens, class_ids, attn=self._att[-1],
                                                        streams=self._dstreams or None, lazy_log=True, enc_out=enc_out,
                                                        fused=self.attn_fused)
        else:
            adv, _log = losses.generator_loss(self.netsD, self.image_encoder, fine_im, real_labels, words_embs, sent_emb,
                                              match_labels, cap_lens, class_ids, streams=self._dstreams or None, lazy_log=True,
                                              gather_negatives=self.gather_negatives, enc_out=enc_out)
        return adv + self._pixel_kl(fake_imgL, fine_im, mu, logvar, hr_pyramid)

    def _encode_early(self, image):
        """`self.image_encoder(image)` on the encoder's own stream, forked from the current one (the image is ready there); the
        caller joins with `_encode_join` before it uses the outputs.  None when the early form is off."""
        if self._encst is None:
            return None
        main = torch.cuda.current_stream(self.device)
        self._encst.wait_stream(main)
        with torch.cuda.stream(self._encst):
            if not torch.cuda.is_current_stream_capturing():
                image.record_stream(self._encst)
            return self.image_encoder(image)

    def _encode_join(self, enc_out):
        if enc_out is None:
            return
        main = torch.cuda.current_stream(self.device)
        main.wait_stream(self._encst)
        if not torch.cuda.is_current_stream_capturing():
            for t in enc_out:
                t.record_stream(main)

    @contextlib.contextmanager
    def _use_packs(self):
        """Scope in which the conv blocks take their packed weights from this trainer's autograd.PackCache."""
        prev, autograd._PACKS = autograd._PACKS, self._packs
        try:
            yield
        finally:
            autograd._PACKS = prev

    @contextlib.contextmanager
    def _wgrad_side(self, stream=None, bucket=None):
        """Scope in which autograd.ConvBnAct issues its weight gradients on `stream` and they land in `bucket` (default: this
        trainer's side stream and the generators' bucket; a discriminator's update passes its own pair).  The stream is joined into
        the CURRENT stream on exit, before anything closes, reduces or reads the bucket; no stream: nothing to do."""
        if bucket is None:
            stream, bucket = self._wside, self.bucket
        if stream is None:
            yield
            return
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        prev = autograd.WGRAD_SIDE.get(idx)
        autograd.WGRAD_SIDE[idx] = stream
        ok = False
        try:
            yield
            ok = True
        finally:
            if prev is None:
                autograd.WGRAD_SIDE.pop(idx, None)
            else:
                autograd.WGRAD_SIDE[idx] = prev
            torch.cuda.current_stream(self.device).wait_stream(stream)          # the join comes first ...
            if not ok:
                autograd._ADOPTED.clear()
        # ... then the check that autograd adopted every side-stream gradient in place.  A failure means the step's gradients
        # are INVALID (an accumulation kernel read a slot the side stream was still writing): the bucket is zeroed so that
        # nothing downstream (all-reduce, optimizer) can consume them, and the error propagates - the caller skips the step.
        try:
            autograd.check_adopted()
        except Exception:
            bucket.flat.zero_()
            raise

    @contextlib.contextmanager
    def _frozen_discriminators(self):
        """Scope in which the discriminators only pass the gradient through to the images: the generator loss runs through them,
        but their own parameter gradients would be discarded (the next discriminator update zeroes its bucket first), so they
        are not computed."""
        d_params = [p for b in self.bucketsD for p in b.params]
        for p in d_params:
            p.requires_grad_(False)
        try:
            yield
        finally:
            for p in d_params:
                p.requires_grad_(True)

    # ------------------------------------------------------------------ updates replayed from hipGraphs
    @staticmethod
    def _opt_key(o):
        """What a captured optimizer step has baked in: the optimizer object, the addresses of its moment / step tensors (a
        load_state_dict replaces them) and its scalar hyper-parameters."""
        first = o.param_groups[0]["params"][0]
        st = o.state.get(first, {})
        ids = tuple(int(st[k].data_ptr()) for k in ("exp_avg", "exp_avg_sq", "step") if torch.is_tensor(st.get(k)))
        return (id(o), ids) + tuple((g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) for g in o.param_groups)

    @staticmethod
    def _bump(tensors):
        """A replayed (or fused-Adam) update wrote parameters and running statistics without telling autograd's version counters,
        which every cache of derived tensors keys on (util._FusedParams, PackCache.get, ...)."""
        torch.autograd.graph.increment_version(tensors)

    def _capture_update(self, buf, refresh, bucket, stream, hyper, loss_fn, finish, message, before=()):
        """One optimizer update captured for replay (nothing executes here: stream capture records).  `buf` holds the static input
        buffers, clones the caller made; `refresh` names those that take new values before every replay (`_load`: one copy).
        The segments, in one memory pool, recorded on `stream` unless they name their own:
            `before`  [(name, stream, fn)], ahead of the update (a stream other than `stream` is forked from it and joined back);
            "fb"      zero `bucket`, `loss_fn()` -> the loss (forward, loss, backward: gradients in place), close the bucket;
            -- the bucket's all-reduce, eager, when there is more than one rank (`_replay_update`) --
            "opt"     `finish()`: the optimizer and whatever follows it      (one rank: the tail of "fb", buf["opt"] stays None).
        `hyper` is what the capture bakes in beside the shapes (`_opt_key`): whoever keeps the capture drops it when that changes.
        Returns `buf` with the graphs and the loss buffer "err" - or False after a failure: the bucket is closed if it was open,
        `message` says why, and the update stays eager (the eager path is always there)."""
        split = dp_world() > 1                               # the all-reduce sits between the two segments
        pool = torch.cuda.graph_pool_handle()
        buf.update(hyper=hyper, opt=None, dst=[t for k in refresh for t in (buf[k] if isinstance(buf[k], list) else [buf[k]])])
        opened, loss = False, None                           # (the loss, and with it its autograd graph, lives until the capture is over)

        def record(name, fn, st=stream):
            buf[name] = torch.cuda.CUDAGraph()
            if st is not stream:
                st.wait_stream(stream)
            with torch.cuda.graph(buf[name], stream=st, pool=pool):
                fn()
            if st is not stream:
                stream.wait_stream(st)

        def fb():
            nonlocal opened, loss
            bucket.begin_step()
            opened = True
            loss = loss_fn()
            bucket.end_step()
            opened = False
            if not split:
                finish()
            buf["err"] = loss.detach()

        try:
            for name, st, fn in before:
                record(name, fn, st)
            record("fb", fb)
            if split:
                record("opt", finish)
        except Exception as ex:                               # noqa: BLE001
            warnings.warn(message % (type(ex).__name__, ex))
            if opened:
                bucket.end_step()                             # close whatever begin_step opened
            return False
        return buf

    @staticmethod
    def _load(cap, srcs):
        with torch.no_grad():
            torch._foreach_copy_(cap["dst"], srcs)

    def _replay_update(self, cap, bucket, bump):
        """Segments "fb" [-> all-reduce] -> "opt" of a captured update on the current stream; returns the loss (a buffer of the
        capture: valid until the next replay)."""
        cap["fb"].replay()
        if cap["opt"] is not None:
            bucket.all_reduce_mean()
            cap["opt"].replay()
        self._bump(bump)
        return cap["err"]

    def reset_d_graphs(self):
        """Forget the captured updates (they are also dropped by themselves when an optimizer's hyper-parameters or state
        tensors change); the next steps capture again."""
        self._dgraphs = [None] * len(self.netsD)
        self._ggraphs = {}

    def _d_update(self, i, graphed, fake, real, sent, real_labels, fake_labels):
        """Discriminator i's update on the current stream (the discriminator's own): zero its bucket, forward on (real,
        fake.detach()), loss, backward, all-reduce, Adam.  `graphed`: from its hipGraphs (`_capture_update`, captured on first use;
        the loss returned is then a buffer of the capture).  A batch of another shape, or a capture that failed once, takes the
        eager update."""
        d, b, o = self.netsD[i], self.bucketsD[i], self.optsD[i]

        def loss_backward(real, fake, sent, rl, fl):
            e = losses.discriminator_loss(d, real, fake, sent, rl, fl)
            with self._wgrad_side(self._dwside[i] if self._dwside else None, b):
                e.backward()
            return e

        g = self._dgraphs[i] if graphed else False
        if g and g["hyper"] != self._opt_key(o):
            g = self._dgraphs[i] = None                     # lr / betas / eps / the moment tensors changed since the capture: capture again
        if g and (tuple(fake.shape) != tuple(g["fake"].shape) or tuple(sent.shape) != tuple(g["sent"].shape)):
            g = False
        if g is None:
            buf = {"fake": fake.detach().clone(), "real": real.clone(), "sent": sent.detach().clone(),
                   "rl": real_labels.clone(), "fl": fake_labels.clone()}
            g = self._dgraphs[i] = self._capture_update(
                buf, ("fake", "real", "sent"), b, self._dstreams[i], self._opt_key(o),
                lambda: loss_backward(buf["real"], buf["fake"], buf["sent"], buf["rl"], buf["fl"]), o.step,
                "discriminator %d: the update could not be captured (%%s: %%s); it stays eager" % i)
        if not g:
            b.begin_step()
            e = loss_backward(real, fake, sent, real_labels, fake_labels)
            b.end_step()
            b.all_reduce_mean()
            o.step()
            self._bump(self._d_bump[i])
            return e
        self._load(g, [fake.detach(), real, sent.detach()])
        return self._replay_update(g, b, self._d_bump[i])

    # ------------------------------------------------------------------ the generators' update from hipGraphs
    def _g_key(self, gan, LR, words_embs, cap_lens, class_ids):
        key = (bool(gan), tuple(LR.shape), int(words_embs.shape[2]), dp_world())
        if self.image_encoder is not None:
            # the DAMSM kernels take the caption lengths (and the class mask) as launch arguments: part of what a capture bakes in
            key += (tuple(int(v) for v in cap_lens),
                    None if class_ids is None else tuple(int(v) for v in np.asarray(class_ids).ravel()))
        return key

    def _g_graphs(self, gan, LR, LRb, hr_pyramid, words_embs, sent_emb, mask, cap_lens, class_ids):
        """The captured update for this step's shapes: a dict of graphs and their static buffers, or None = take the eager step
        (warm-up, switched off, a configuration that needs a collective inside the loss, or a capture that failed).  A change of
        the optimizer's state or hyper-parameters drops every shape's capture, the failed ones included."""
        use = self._policy.replays(self._gsteps)
        self._gsteps += 1
        if not use or self._attn_losses or (self.image_encoder is not None and self.gather_negatives and dp_world() > 1):
            # (DAMSM on the gathered global batch all-gathers inside generator_loss; the attention-guided losses are not captured yet)
            return None
        hyper = self._opt_key(self.opt) + (self.ema_decay, self.cycle, self.perceptual_weight)
        if hyper != self._ghyper:
            self._ggraphs, self._ghyper = {}, hyper
        key = self._g_key(gan, LR, words_embs, cap_lens, class_ids)
        g = self._ggraphs.get(key)
        if g is None:
            g = self._ggraphs[key] = self._capture_g(gan, LR, LRb, hr_pyramid, words_embs, sent_emb, mask, cap_lens, class_ids)
        return g or None

    def _pixel_kl(self, fake_imgL, fine_im, mu, logvar, hr_pyramid):
        base = self._pixel_kl_base(fake_imgL, fine_im, mu, logvar, hr_pyramid)
        if self.perceptual is not None and self.perceptual_weight > 0:
            base = base + self.perceptual_weight * self.perceptual(fine_im[-1], hr_pyramid[-1]).mean()
        if self.cycle > 0:          # (cycle == 0: CycleMSE is not called and the loss is the expression it always was)
            return base + self.cycle * (losses.CycleMSE(fake_imgL, self._lr_in, fused=self.cycle_fused) +
                                        losses.CycleMSE(fine_im, self._lr_in, fused=self.cycle_fused))
        return base

    def _pixel_kl_base(self, fake_imgL, fine_im, mu, logvar, hr_pyramid):
        if self.pixel_loss == "weight_mse":
            return (losses.weight_MSE(fake_imgL, hr_pyramid, self._att, fused=self.attn_fused)[0] +
                    losses.weight_MSE(fine_im, hr_pyramid, self._att, fused=self.attn_fused)[0] + losses.KL_loss(mu, logvar))
        return losses.MSE(fake_imgL, hr_pyramid) + losses.MSE(fine_im, hr_pyramid) + losses.KL_loss(mu, logvar)

    def _loss_from(self, fake_imgL, fine_im, mu, logvar, words_embs, sent_emb, cap_lens, hr_pyramid, class_ids):
        """The generator-only step's loss on the networks' outputs (see `loss`)."""
        errG = self._pixel_kl(fake_imgL, fine_im, mu, logvar, hr_pyramid)
        if self.image_encoder is not None:
            region_features, cnn_code = self.image_encoder(fine_im[-1])
            if self.reweight:
                self._check_reweight()
                B = sent_emb.shape[0]
                labels = torch.arange(B, device=sent_emb.device)
                w0, w1, _ = losses.words_reweight_loss(region_features, words_embs, labels, cap_lens, class_ids, B, self._att[-1],
                                                       fused=self.attn_fused)
                s0, s1 = losses.sent_loss(cnn_code, sent_emb, labels, class_ids, B)
                scale = 1
            else:
                w0, w1, s0, s1, scale, _ = losses.damsm_terms(region_features, cnn_code, words_embs, sent_emb, cap_lens, class_ids,
                                                              gather=self.gather_negatives)
            errG = errG + (w0 + w1 + s0 + s1) * (cfg.TRAIN.SMOOTH.LAMBDA * scale)
        return errG

    def _g_backward(self, errG, early=True):
        """errG.backward() with the packs and the weight-gradient side stream; the discriminators only pass the gradient through
        to the images (their own parameter gradients would be discarded: not computed)."""
        if early:
            self._arm_early()
        else:
            self._early, self._early_left = None, -1
        trunk = getattr(self.image_encoder, "_hip_trunk", None)
        if trunk is not None:
            trunk.bwd_stream = torch.cuda.current_stream(self.device)      # (inception.TrunkFn.backward: where the walk belongs)
        with self._use_packs(), self._wgrad_side():
            errG.backward()

    def _g_finish(self, captured=False):
        """What follows the gradient all-reduce: Adam, the re-pack of every cached weight pack, the EMA of the parameters."""
        self.opt.step()
        if captured:
            if self._packs is not None:
                self._packs.repack_captured(self._gpack)
        elif self._packs is not None:
            self._packs.repack(force=True)      # the optimizer has just run: every pack is stale, whatever the version counters say
        with torch.no_grad():
            torch._foreach_mul_(self.avg_param_G, self.ema_decay)
            torch._foreach_add_(self.avg_param_G, [p.data for p in self.params], alpha=1.0 - self.ema_decay)
        if captured and self._packs is not None:
            torch.cuda.current_stream(self.device).wait_stream(self._gpack)      # join the pack branch before the capture ends

    def _g_loss_backward(self, gan, nets, LR, LRb, words_embs, sent_emb, mask, cap_lens, hr_pyramid, class_ids, enc_out=None,
                         early=True):
        """With the generators' bucket open: [both generators forward,] the loss, backward.  G/D alternation: `nets`, the
        generators' outputs, were computed ahead of the discriminator updates, and the loss runs through the frozen
        discriminators.  Returns (errG, nets)."""
        if gan:
            with self._frozen_discriminators():
                errG = self.g_loss(*nets, words_embs, sent_emb, cap_lens, hr_pyramid, class_ids, enc_out=enc_out)
                self._g_backward(errG, early)
        else:
            with self._use_packs():
                nets = self._forward_nets(LR, LRb, words_embs, sent_emb, mask)
                errG = self._loss_from(*nets, words_embs, sent_emb, cap_lens, hr_pyramid, class_ids)
            self._g_backward(errG, early)
        return errG, nets

    def _capture_g(self, gan, LR, LRb, hr_pyramid, words_embs, sent_emb, mask, cap_lens, class_ids):
        """Capture the generators' update for one batch shape (`_capture_update`; `_step` replays).  Its segments, the autograd graph
        of "fwd" alive while "fb" is recorded:
            "fwd" (G/D alternation only)  both generators forward - the discriminator updates run between it and "fb";
            "enc" (TGSR_ENC_EARLY)        the image encoder's forward, captured on ITS stream as the origin (its branch forks are then
                                          plain diamonds) and replayed beside the discriminators' graphs; its autograd node stays alive;
            "fb"   zero the bucket, [forward,] losses, backward (weight gradients on the side branch), gradients in place;
            "opt"  fused Adam, every weight pack re-derived (a branch of its own, joined before the capture ends), EMA."""
        buf = {"LR": LR.clone(), "LRb": LRb.clone(), "hr": [h.clone() for h in hr_pyramid], "words": words_embs.clone(),
               "sent": sent_emb.clone(), "mask": mask.clone(), "fwd": None, "enc": None}
        cap_lens = [int(v) for v in cap_lens]
        if self._packs is not None:
            self._packs.settle(self.device)
        live = []                                            # the networks' outputs, alive until the capture is over
        before = []

        def fwd():
            with self._use_packs():
                live.append(self._forward_nets(buf["LR"], buf["LRb"], buf["words"], buf["sent"], buf["mask"]))
            buf["fine"] = live[0][1]

        def enc():
            buf["enc_out"] = self.image_encoder(buf["fine"][len(self.netsD) - 1])

        def loss_backward():
            errG, nets = self._g_loss_backward(gan, live[0] if gan else None, buf["LR"], buf["LRb"], buf["words"], buf["sent"], buf["mask"],
                                               cap_lens, buf["hr"], class_ids, enc_out=buf.get("enc_out"), early=False)
            live.append(nets)
            return errG

        if gan:
            before.append(("fwd", self._gcap, fwd))
            if self._encst is not None:
                before.append(("enc", self._encst, enc))
        return self._capture_update(buf, ("LR", "LRb", "words", "sent", "mask", "hr"), self.bucket, self._gcap, self._ghyper,
                                    loss_backward, lambda: self._g_finish(captured=True),
                                    "the generators' update could not be captured (%s: %s); it stays eager", before)

    def _d_updates(self, fine_im, hr_pyramid, sent_emb):
        """Every discriminator's update on (real, fake.detach()): each on a stream of its own - replayed from its hipGraphs once
        the step has run GRAPH_D_WARMUP times."""
        graphed = bool(self._dstreams) and self._graph_d and self._dsteps >= GRAPH_D_WARMUP
        self._dsteps += 1
        B = sent_emb.shape[0]
        real_labels, fake_labels, _ = prepare_labels(B, self.device)
        if not self._dstreams:
            return [self._d_update(i, False, fine_im[i], hr_pyramid[i], sent_emb, real_labels, fake_labels)
                    for i in range(len(self.netsD))]
        # the three discriminators are independent of each other: each one's forward, backward, all-reduce and Adam
        # step run on a stream of their own (the 64^2 / 128^2 discriminators' layers leave most CUs idle)
        main = torch.cuda.current_stream(self.device)
        errsD = []
        for i, st in enumerate(self._dstreams):
            st.wait_stream(main)
            with torch.cuda.stream(st):
                for t in (fine_im[i], hr_pyramid[i], sent_emb):
                    t.record_stream(st)
                errsD.append(self._d_update(i, graphed, fine_im[i], hr_pyramid[i], sent_emb, real_labels, fake_labels))
        for st in self._dstreams:
            main.wait_stream(st)
        return errsD

    def _step(self, gan, captions, cap_lens, LR, LRb, hr_pyramid, class_ids):
        """One step of either kind: (errG, [errD_i]), detached (buffers of the captures when the step is replayed).  gan: both
        generators forward once, every discriminator's update on (real, fake.detach()) - the image encoder's forward beside them
        when it runs early - then the generators' update through the UPDATED discriminators on the same fake images."""
        k = self._gsteps
        self._policy.begin(k)
        words_embs, sent_emb, mask = self._text(captions, cap_lens)
        g = self._g_graphs(gan, LR, LRb, hr_pyramid, words_embs, sent_emb, mask, cap_lens, class_ids)
        errsD, nets, enc_out = [], None, None
        if g is not None:
            self._load(g, [LR, LRb, words_embs, sent_emb, mask] + list(hr_pyramid))
            if self._packs is not None:
                self._packs.settle(self.device)
            if gan:
                g["fwd"].replay()
                if g["enc"] is not None:                        # the image encoder's forward beside the discriminator updates
                    self._encst.wait_stream(torch.cuda.current_stream(self.device))
                    with torch.cuda.stream(self._encst):
                        g["enc"].replay()
                errsD = self._d_updates(g["fine"], g["hr"], g["sent"])
                if g["enc"] is not None:
                    torch.cuda.current_stream(self.device).wait_stream(self._encst)
            self._early, self._early_left = None, -1
            errG = self._replay_update(g, self.bucket, self._g_bump)
            if self._packs is not None:
                self._packs.mark_fresh()
            self._policy.end(k, True)
            return errG, [e.detach() for e in errsD]
        if gan:
            with self._use_packs():
                nets = self._forward_nets(LR, LRb, words_embs, sent_emb, mask)
            enc_out = self._encode_early(nets[1][len(self.netsD) - 1])          # beside the discriminator updates
            errsD = self._d_updates(nets[1], hr_pyramid, sent_emb)
            self._encode_join(enc_out)
        self._zero(self.bucket)
        try:
            errG, _nets = self._g_loss_backward(gan, nets, LR, LRb, words_embs, sent_emb, mask, cap_lens, hr_pyramid, class_ids, enc_out)
        finally:
            self.bucket.end_step()               # also after a failed step: `.grad` views restored, slots closed
        self._all_reduce()
        self._g_finish()
        self._bump(self._g_bump)
        self._policy.end(k, False)
        return errG.detach(), [e.detach() for e in errsD]

    def step_gan(self, captions, cap_lens, LR, LRb, hr_pyramid, class_ids=None):
        """One G/D alternation: forward the generators once; update every discriminator on (real, fake.detach());
        then update the generators through the UPDATED discriminators on the same fake images.  Returns
        (errG, [errD_i]) as detached tensors (buffers of the captures when the step is replayed: valid until the next step)."""
        return self._step(True, captions, cap_lens, LR, LRb, hr_pyramid, class_ids)

    def step(self, captions, cap_lens, LR, LRb, hr_pyramid, class_ids=None):
        """forward + backward + gradient all-reduce (if distributed) + Adam + EMA.  Returns the loss tensor.  With
        discriminators this is `step_gan` (the generator loss is returned).  After GRAPH_G_WARMUP eager steps the update is
        replayed from hipGraphs (`_capture_g`), bit-identical to the eager one."""
        return self._step(bool(self.netsD), captions, cap_lens, LR, LRb, hr_pyramid, class_ids)[0]

    # ------------------------------------------------------------------ validation, snapshots, resume
    @contextlib.contextmanager
    def _eval_weights(self, ema):
        """Scope in which both generators are in eval mode and - `ema` - hold the EMA weights `avg_param_G`, copied IN PLACE
        into the parameters (their addresses, which the flat optimizer and the captured graphs are bound to, do not change).
        On exit everything is as it was: the parameters bit for bit, the training modes, the random generators' states, and the
        weight packs of the PackCache (derived from the restored values: still valid, so they are not marked stale)."""
        cuda = self.device.type == "cuda"
        nets = (self.netGL, self.netGH)
        modes = [m.training for m in nets]
        rng_cpu = torch.get_rng_state()
        rng_dev = torch.cuda.get_rng_state(self.device) if cuda else None
        fresh = None
        if self._packs is not None:
            self._packs.settle(self.device)                  # a pending re-pack reads the parameters: it comes first
            fresh = [e for e in self._packs.entries.values() if e[4] == e[0]._version]
        backup = None
        try:
            with torch.no_grad():
                if ema:
                    backup = [p.detach().clone() for p in self.params]
                    torch._foreach_copy_([p.data for p in self.params], self.avg_param_G)
                    self._bump(self._g_bump)                           # the eval modules' folded / packed weights key on the version counters
            for m in nets:
                m.eval()
            yield
        finally:
            with torch.no_grad():
                if backup is not None:
                    torch._foreach_copy_([p.data for p in self.params], backup)
                    self._bump(self._g_bump)
            for m, mode in zip(nets, modes):
                m.train(mode)
            if fresh is not None:
                for e in fresh:
                    e[4] = e[0]._version
            torch.set_rng_state(rng_cpu)
            if rng_dev is not None:
                torch.cuda.set_rng_state(rng_dev, self.device)

    @torch.no_grad()
    def evaluate(self, batches, ema=True, shave=0, max_batches=None, r_precision=None, generator=None, ensemble=1, fid=None,
                 kid=None, niqe=None, lpips=None):
        """Score a validation set: `batches` yields (captions, cap_lens, LR, LRb, hr_pyramid); the generators run in eval mode
        (SRPipeline.from_modules over this trainer's modules, no copies) with the EMA weights (`ema`, the ones `snapshot` saves by
        default) or the current ones, and every output scale is scored against hr_pyramid[k] on the device (tgsr_amd.metrics:
        PSNR / RMSE on RGB and Y, SSIM on Y, `shave` border pixels removed) - no synchronisation per batch, one at the end.
        Returns {"fine": [per scale], "fake": [per scale]}, per scale {"psnr": [N], "rmse", "psnr_y", "rmse_y", "ssim_y", "n": N,
        "mean": {...}} over the N images seen.  Afterwards the trainer is exactly as it was (`_eval_weights`).
        ensemble=8 scores the geometric self-ensemble (SRPipeline.self_ensemble: the mean over the eight flips and rotations, the
        "+" rows of an SR table) in place of the plain forward; everything else is unchanged.
        Every further score is off by default (None: nothing of it happens), reads the finest `fine` image and the finest
        ground-truth image of every batch, and is kept by one accumulator, which states the rest:
        `r_precision` = K - is the output consistent with its caption?  The batches carry `class_ids` as a sixth element, the image
          goes through `image_encoder` (required); the dict gains "r_precision": {"sent": ..., "words": ...}, each
          retrieval.r_precision over the images seen (retrieval.Gallery) against sample_candidates(class_ids, K, generator): the own
          caption and K - 1 captions of other classes.
        `fid` = True, a FeatureMoments or the path of a saved one, `kid` = True or {"subsets": ..., "subset_size": ...} - does the
          output look like a real image?  Both images go through `image_encoder.run_trunk` (required; tgsr_amd.featdist states the
          feature space), only `pooled` is kept; with saved statistics alone the ground truth's walks are skipped, and with
          `r_precision` as well the SR image is walked once: run_trunk, then heads.  The dict gains "fid": {"fine": the Frechet
          distance, "n": the images seen} and "kid": featdist.kernel_distance's result, subsets drawn from `generator` after
          r_precision's candidates (featdist.RealismScores).
        `niqe` = True (the model is fitted from the ground-truth images seen), a NIQEModel or the path of one - how natural does each
          image look on its own?  Lower is better; `shave` applies; the finest scale needs 96 pixels on a side after it.  The dict
          gains "niqe": {"fine": [N], "hr": [N], "mean": {"fine", "hr"}, "n": N} (niqe.NIQEScores).
        `lpips` = a tgsr_amd.lpips.LPIPS or the path of a saved one - the learned perceptual distance to the ground truth (lower is
          better).  Both images are scored as the saved PNGs would be: after the quantisation PSNR is scored on (`to_uint8`, mapped
          back by u / 127.5 - 1), so the figure is the one a reader of the files computes; `shave` is NOT applied; 16 pixels on a
          side at least.  The dict gains "lpips": {"fine": [N], "mean", "n": N, "per_layer": [5][N]} (lpips.PerceptualScores), rows
          gathered in rank order.  A figure comparable with published LPIPS needs that package's trained weights, which are not shipped.
        Data parallel: every rank passes ITS batches; the PSNR / SSIM and NIQE rows are gathered in rank order and the moments behind
        "fid" and niqe=True's fit are all-reduced, so every rank returns the same of those; "r_precision" and "kid" score the
        calling rank's items only (region features and feature banks are not gathered across ranks)."""
        if getattr(self, "_eval_pipe", None) is None:
            self._eval_pipe = SRPipeline.from_modules(self.text_encoder, self.netGL, self.netGH, device=self.device)
        if r_precision is not None and self.image_encoder is None:
            raise ValueError("evaluate(r_precision=%r) needs the trainer's image_encoder" % (r_precision,))
        if ensemble not in (1, 8):
            raise ValueError("evaluate: ensemble is 1 or 8 (the eight flips and rotations), got %r" % (ensemble,))
        fid, kid = featdist.realism_args(fid, kid)
        if (fid is not None or kid is not None) and self.image_encoder is None:
            raise ValueError("evaluate(fid=%r, kid=%r) needs the trainer's image_encoder" % (fid, kid))
        realism = featdist.RealismScores(fid, kid, self.device) if fid is not None or kid is not None else None
        naturalness = niqe_mod.NIQEScores(niqe, shave, self.device) if niqe is not None and niqe is not False else None
        perceptual = lpips_mod.PerceptualScores(lpips, self.device) if lpips is not None else None
        gallery = retrieval.Gallery() if r_precision is not None else None
        forward = self._eval_pipe if ensemble == 1 else self._eval_pipe.self_ensemble
        book = metrics.ScoreBook(shave)
        with torch.cuda.device(self.device), self._eval_weights(ema):
            for k, batch in enumerate(batches):
                if gallery is None:
                    captions, cap_lens, LR, LRb, hr_pyramid = batch
                else:
                    captions, cap_lens, LR, LRb, hr_pyramid, class_ids = batch
                if max_batches is not None and k >= max_batches:
                    break
                out = forward(captions, cap_lens, LR, LRb)
                sr, hr = out["fine"][-1], hr_pyramid[-1]
                if realism is not None:
                    trunk_feats, pooled = self.image_encoder.run_trunk(sr)
                    realism.add(pooled, featdist.pooled_of_truth(self.image_encoder, hr) if realism.needs_truth else None)
                if gallery is not None:
                    words_embs, sent_emb, _mask = self._text(captions, cap_lens)
                    feats, code = self.image_encoder.heads(trunk_feats, pooled) if realism is not None else self.image_encoder(sr)
                    gallery.add(feats, code, words_embs, sent_emb, cap_lens, class_ids=class_ids)
                if naturalness is not None:
                    naturalness.add(sr, hr)
                if perceptual is not None:
                    perceptual.add(sr, hr)
                for name in ("fine", "fake"):
                    if len(out[name]) != len(hr_pyramid):
                        raise ValueError("evaluate: %d %s images against %d ground-truth scales"
                                         % (len(out[name]), name, len(hr_pyramid)))
                    for i, truth in enumerate(hr_pyramid):
                        book.add((name, i), out[name][i].contiguous(), truth.contiguous())
        with torch.cuda.device(self.device):
            res = book.all_gather().result()
            if not res:
                raise ValueError("evaluate: no validation batch")
            nscales = 1 + max(i for _name, i in res)
            scores = {name: [res[name, i] for i in range(nscales)] for name in ("fine", "fake")}
            if gallery is not None:
                cand = retrieval.sample_candidates(gallery.class_ids, int(r_precision), generator)
                items = gallery.cat()
                scores["r_precision"] = {mode: retrieval.r_precision(*items, cand, mode=mode) for mode in retrieval.MODES}
            if realism is not None:
                scores.update(realism.result(generator))
            if naturalness is not None:
                scores["niqe"] = naturalness.result()
            if perceptual is not None:
                scores["lpips"] = perceptual.result()
        return scores

    def snapshot_due(self, epoch, max_epoch=None):
        return snapshot_due(epoch, max_epoch)

    @staticmethod
    def snapshot_paths(model_dir, epoch):
        """(`netG_epoch_%d.pth`, the same with 'netG' -> 'netGH'): the pair trainer_objective.py:90-93 loads."""
        name = "netG_epoch_%d.pth" % epoch
        return os.path.join(model_dir, name), os.path.join(model_dir, name.replace("netG", "netGH"))

    def _state_dicts(self, ema):
        """(G_SR_NET_low's, NetG_highweight's) state_dicts, detached copies; `ema`: the parameters' entries are the EMA weights."""
        sds, k = [], 0
        for m in (self.netGL, self.netGH):
            sd = {name: v.detach().clone() for name, v in m.state_dict().items()}
            for name, _p in m.named_parameters():
                if ema and name in sd:
                    sd[name] = self.avg_param_G[k].detach().clone()
                k += 1
            sds.append(sd)
        return sds

    def snapshot(self, model_dir, epoch, ema=True):
        """`netG_epoch_%d.pth` (G_SR_NET_low) and `netGH_epoch_%d.pth` (NetG_highweight): state_dicts only, the keys of the shipped
        checkpoints - what the reference's caller (trainer_objective.py:90-93) and SRPipeline.load_state_dicts load strictly.
        `ema` (default): the EMA weights `avg_param_G` with the current running statistics, else the current weights.  No
        optimizer state (the reference saves none).  Under data parallelism call it on rank 0."""
        os.makedirs(model_dir, exist_ok=True)
        pl, ph = self.snapshot_paths(model_dir, epoch)
        sd_l, sd_h = self._state_dicts(ema)
        torch.save(sd_l, pl)
        torch.save(sd_h, ph)
        return pl, ph

    @staticmethod
    def resume_epoch(net_g):
        """The epoch to continue from, out of a snapshot's file name: the digits behind the last '_', + 1; '' -> 0."""
        if net_g == '':
            return 0
        return int(net_g[net_g.rfind('_') + 1:net_g.rfind('.')]) + 1

    def resume(self, net_g=None):
        """Load `cfg.TRAIN.NET_G` (a netG snapshot) and NetG_highweight from the same name with 'netG' -> 'netGH'
        (trainer_objective.py:90-93), IN PLACE - parameter addresses, and with them the flat optimizer's views and the captured
        graphs, stay valid; the EMA copy restarts from the loaded weights, the version counters move and every cached weight
        pack is re-derived.  Optimizer moments are left as they are (none are saved).  Returns the epoch to continue from."""
        net_g = cfg.TRAIN.NET_G if net_g is None else net_g
        start = self.resume_epoch(net_g)
        if net_g == '':
            return 0
        d, base = os.path.split(net_g)
        sd_l = torch.load(net_g, map_location=self.device)
        sd_h = torch.load(os.path.join(d, base.replace('netG', 'netGH')), map_location=self.device)
        if self._packs is not None:
            self._packs.settle(self.device)
        self.netGL.load_state_dict(sd_l, strict=True)
        self.netGH.load_state_dict(sd_h, strict=True)
        with torch.no_grad():
            torch._foreach_copy_(self.avg_param_G, [p.data for p in self.params])
        self._bump(self._g_bump)
        if self._packs is not None:
            self._packs.repack(force=True)
        return start


class DAMSMTrainer:
    """pretrain_DAMSM.py:48-125, 262-284: joint training of RNN_ENCODER and the CNN_ENCODER heads on
    words_loss + sent_loss.  Every gradient comes from HIP kernels: DAMSM backward (tgsr_damsm_words_bwd), LSTM BPTT
    (tgsr_bilstm_bwd) and the GEMMs of the heads; the Inception trunk is the Inception blocks themselves (`inception=`: walked
    in training mode on the library's kernels), the caller's frozen module (CNN_ENCODER(trunk=...)) or pre-extracted features
    via `step_features`.  Like the reference: a fresh
    Adam(lr, betas (0.5, 0.999)) per epoch, lr x 0.98 per epoch down to ENCODER_LR / 10, gradient-norm clip
    RNN_GRAD_CLIP on the text encoder only.  Data parallel: one flat gradient bucket, one all-reduce per step; the
    contrastive losses are those of the GLOBAL batch (features and embeddings all-gathered, parallel.gather_damsm_batch;
    `gather_negatives=False` / TGSR_DP_GATHER_NEGATIVES=0: the local shard's negatives only - SURVEY section 8e (2))."""

    def __init__(self, n_words, device="cuda", trunk=None, lr=None, gather_negatives=None, inception=None):
        """`inception`: the Inception-v3 blocks (torchvision's attribute names, e.g. a loaded `models.inception_v3()`): `step(imgs,
        ...)` then walks raw images through the frozen trunk in training mode on the library's kernels (batch-statistics
        BatchNorm, running statistics drifting as in pretrain_DAMSM.py:49-51, 70) and `evaluate` in eval mode; `snapshot` saves
        the drifted statistics with the heads.  Default: `trunk` (a callable images -> (features, pooled)), else nn.Identity."""
        if trunk is not None and inception is not None:
            raise ValueError("DAMSMTrainer: pass `trunk` or `inception`, not both")
        self.device = torch.device(device)
        self.gather_negatives = parallel.GATHER_NEGATIVES if gather_negatives is None else bool(gather_negatives)
        self.text_encoder = RNN_ENCODER(n_words, nhidden=cfg.TEXT.EMBEDDING_DIM).to(self.device).train()
        if inception is not None:
            self.image_encoder = CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM, inception=inception).to(self.device)
        else:
            self.image_encoder = CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM,
                                             trunk=trunk if trunk is not None else torch.nn.Identity()).to(self.device)
        self.image_encoder.train()
        for p in self.image_encoder.frozen_parameters():
            p.requires_grad = False                                  # util.py:274-275
        self.params = list(self.text_encoder.parameters()) + [p for p in self.image_encoder.parameters()
                                                              if p.requires_grad]
        self.bucket = FlatGradBucket(self.params).attach()
        self.base_lr = self.lr = lr or cfg.TRAIN.ENCODER_LR
        self.start_epoch()

    def start_epoch(self):
        """pretrain_DAMSM.py:270: the optimizer (and its moments) is rebuilt every epoch; train() puts both encoders back
        in training mode (:49-50; evaluate() leaves them in eval mode)."""
        self.text_encoder.train()
        self.image_encoder.train()
        self.opt = torch.optim.Adam(self.params, lr=self.lr, betas=(0.5, 0.999))

    # ------------------------------------------------------------------ validation, snapshots, resume
    @torch.no_grad()
    def evaluate_features(self, batches):
        """pretrain_DAMSM.py:133-163 on trunk outputs: `batches` yields (features, pooled, captions, cap_lens, class_ids);
        both encoders in eval mode (and left there, as in the reference), at most 51 batches (`if step == 50: break`),
        returns (s_cur_loss, w_cur_loss) = the summed sentence / word losses divided by the LAST STEP INDEX - the
        reference's `s_total_loss[0] / step` (:160-161), not by the number of batches: N batches (N <= 50) are divided by
        N - 1, a single batch by 0 (inf), 51 or more by 50.  Kept as is: the numbers it prints are the ones a user of
        the reference compares against."""
        self.text_encoder.eval()
        self.image_encoder.eval()
        s_total = torch.zeros((), dtype=torch.float32, device=self.device)
        w_total = torch.zeros((), dtype=torch.float32, device=self.device)
        step = -1
        for step, (features, pooled, captions, cap_lens, class_ids) in enumerate(batches):
            B = captions.shape[0]
            labels = torch.arange(B, device=self.device)
            words_features, sent_code = self.image_encoder.heads(features, pooled)
            words_emb, sent_emb = self.text_encoder(captions, cap_lens, self.text_encoder.init_hidden(B))
            w0, w1, _att = losses.words_loss(words_features, words_emb, labels, cap_lens, class_ids, B)
            s0, s1 = losses.sent_loss(sent_code, sent_emb, labels, class_ids, B)
            w_total += (w0 + w1).detach()
            s_total += (s0 + s1).detach()
            if step == 50:
                break
        if step < 0:
            raise ValueError("evaluate: no validation batch (the reference only evaluates when len(dataloader_val) > 0)")
        s, w = float(s_total), float(w_total)
        return (s / step, w / step) if step > 0 else (float("inf") * (1 if s >= 0 else -1), float("inf") * (1 if w >= 0 else -1))

    @torch.no_grad()
    def evaluate(self, batches):
        """pretrain_DAMSM.py:133-163 with the images through the (frozen) trunk: `batches` yields
        (imgs, captions, cap_lens, class_ids) - imgs = the data loader's real_imgs[-1]."""
        def through_trunk():
            for imgs, captions, cap_lens, class_ids in batches:
                features, pooled = self.image_encoder.run_trunk(imgs)
                yield features, pooled, captions, cap_lens, class_ids
        return self.evaluate_features(through_trunk())

    @torch.no_grad()
    def evaluate_retrieval(self, batches, ks=(1, 5, 10), max_items=None):
        """Retrieval accuracy of the two encoders on a validation set (not in the reference's loop, which prints only the two summed
        losses): `batches` yields what `evaluate` takes, (imgs, captions, cap_lens, class_ids), or what `evaluate_features` takes,
        (features, pooled, captions, cap_lens, class_ids).  Both encoders in eval mode and left there, like `evaluate`.  The region
        features, image codes and text embeddings of every item (at most `max_items`) are gathered on the device and scored as ONE
        gallery by retrieval.retrieval_scores: recall@k and the median rank, image -> text and text -> image, for the sentence and
        the word similarity.  Data parallel: every rank scores the items of ITS batches only (no gather of region features)."""
        self.text_encoder.eval()
        self.image_encoder.eval()
        gallery = retrieval.Gallery()
        with torch.cuda.device(self.device):
            for batch in batches:
                if max_items is not None and len(gallery) >= max_items:
                    break
                if len(batch) == 4:
                    imgs, captions, cap_lens, _cls = batch
                    features, pooled = self.image_encoder.run_trunk(imgs)
                else:
                    features, pooled, captions, cap_lens, _cls = batch
                B = captions.shape[0]
                wf, code = self.image_encoder.heads(features, pooled)
                we, se = self.text_encoder(captions, cap_lens, self.text_encoder.init_hidden(B))
                gallery.add(wf, code, we, se, cap_lens, take=B if max_items is None else min(B, max_items - len(gallery)))
            if not len(gallery):
                raise ValueError("evaluate_retrieval: no validation batch")
            return retrieval.retrieval_scores(*gallery.cat(), ks)

    def snapshot_due(self, epoch, max_epoch=None):
        return snapshot_due(epoch, max_epoch)

    def snapshot(self, model_dir, epoch):
        """pretrain_DAMSM.py:288-291: `image_encoder%d.pth` / `text_encoder%d.pth` state_dicts (no optimizer state: the
        reference rebuilds Adam every epoch anyway).  Under data parallelism call it on rank 0 (parameters are identical
        on every rank after the all-reduced step)."""
        os.makedirs(model_dir, exist_ok=True)
        pi, pt = "%s/image_encoder%d.pth" % (model_dir, epoch), "%s/text_encoder%d.pth" % (model_dir, epoch)
        torch.save(self.image_encoder.state_dict(), pi)
        torch.save(self.text_encoder.state_dict(), pt)
        return pi, pt

    def resume(self, net_e=None):
        """pretrain_DAMSM.py:172-186: load `cfg.TRAIN.NET_E` (a text_encoder snapshot), the image encoder from the same
        name with 'text_encoder' -> 'image_encoder', and take the epoch to continue from out of the file name
        (`istart = rfind('_') + 8`: the digits behind 'text_encoder').  Returns start_epoch = that epoch + 1; the learning
        rate restarts at ENCODER_LR as in the reference (the decayed value is not saved)."""
        net_e = cfg.TRAIN.NET_E if net_e is None else net_e
        if net_e == '':
            return 0
        self.text_encoder.load_state_dict(torch.load(net_e, map_location=self.device))
        self.image_encoder.load_state_dict(torch.load(net_e.replace('text_encoder', 'image_encoder'),
                                                      map_location=self.device))
        istart, iend = net_e.rfind('_') + 8, net_e.rfind('.')
        self.start_epoch()
        return int(net_e[istart:iend]) + 1

    def end_epoch(self):
        """pretrain_DAMSM.py:283-284."""
        if self.lr > self.base_lr / 10.:
            self.lr *= 0.98

    def loss_from_features(self, features, pooled, captions, cap_lens, class_ids=None):
        B = captions.shape[0]
        labels = torch.arange(B, device=self.device)
        words_features, sent_code = self.image_encoder.heads(features, pooled)
        words_emb, sent_emb = self.text_encoder(captions, cap_lens, self.text_encoder.init_hidden(B))
        # data parallel (gather_negatives): the losses of the GLOBAL batch, identical on every rank; step_features multiplies by
        # `_bw_scale` = world for backward (the bucket's all-reduce averages what a replicated loss needs summed)
        w0, w1, s0, s1, scale, att = losses.damsm_terms(words_features, sent_code, words_emb, sent_emb, cap_lens, class_ids,
                                                        gather=self.gather_negatives)
        self._bw_scale = scale
        return w0 + w1 + s0 + s1, (w0.detach(), w1.detach(), s0.detach(), s1.detach()), att

    def step_features(self, features, pooled, captions, cap_lens, class_ids=None):
        """One optimisation step on trunk outputs (features [B,768,17,17], pooled [B,2048]).  Returns the loss."""
        self.bucket.flat.zero_()
        for p, v in zip(self.bucket.params, self.bucket.views):
            p.grad = v
        loss, _parts, _att = self.loss_from_features(features, pooled, captions, cap_lens, class_ids)
        (loss * self._bw_scale if self._bw_scale != 1 else loss).backward()
        self.bucket.all_reduce_mean()
        torch.nn.utils.clip_grad_norm_(self.text_encoder.parameters(), cfg.TRAIN.RNN_GRAD_CLIP)   # :96-97
        self.opt.step()
        return loss.detach()

    def step(self, imgs, captions, cap_lens, class_ids=None):
        """pretrain_DAMSM.py:66-98 with the image through the (frozen) trunk."""
        with torch.no_grad():
            features, pooled = self.image_encoder.run_trunk(imgs)
        return self.step_features(features, pooled, captions, cap_lens, class_ids)
