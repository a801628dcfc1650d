"""Training-method stand-in behind the reference's plugin API
(`task.build_method(model=, datamodule=, params=, ckp_path=, local_rank=, use_ddp=, use_fp16=)`,
scripts/train.py:65-76; optimiser groups and schedule of img_based/method.py:235-285 /
video_based/method.py:291-341; loss weighting `params.<loss>_w`, clipping, AMP switch and the
per-step hook as nerv's BaseMethod does them).

The reference delegates the loop to nerv's trainer (logging, wandb, Slurm requeue ...), which is out
of scope; this class keeps the part of it that IS the hot path: one process per
GPU, fused clip+Adam over the flat arena, gradient all-reduce of the arena over RCCL, optional HIP
graph replay of the whole step.
"""
import os

import torch

from . import parallel
from .optim import FusedAdam, GraphedTrainStep


class SyntheticDataModule:
    """`build_dataset` stand-in: seeded random images in [-1, 1] of the configured shape
    (datasets themselves are out of scope; SURVEY section 8(d) defines this synthetic input)."""

    def __init__(self, params, steps_per_epoch=8, frames=None, device='cuda', seed=1234):
        self.params = params
        self.steps_per_epoch = steps_per_epoch
        self.frames = frames
        self.device = device
        self.seed = seed
        self.rank = int(os.environ.get('RANK', 0))

    def __len__(self):
        return self.steps_per_epoch

    def train_loader(self, epoch=0):
        B = self.params.train_batch_size
        res = self.params.resolution
        H, W = (res, res) if isinstance(res, int) else res
        g = torch.Generator().manual_seed(self.seed + 1000 * epoch + self.rank)
        for _ in range(self.steps_per_epoch):
            shape = (B, 3, H, W) if self.frames is None else (B, self.frames, 3, H, W)
            yield {'img': (torch.randn(shape, generator=g) * 0.5).clamp_(-1, 1).to(self.device)}


class SyntheticSlotsDataModule:
    """`build_dataset` stand-in of the vp_vqa task: seeded random slots [B, history + rollout, N, D] (the Physion slots
    reader is out of scope; the model consumes pre-extracted slots, vp_vqa/datasets/physion.py)."""

    def __init__(self, params, steps_per_epoch=8, device='cuda', seed=1234):
        self.params, self.steps_per_epoch, self.device, self.seed = params, steps_per_epoch, device, seed
        self.rank = int(os.environ.get('RANK', 0))

    def __len__(self):
        return self.steps_per_epoch

    def train_loader(self, epoch=0):
        p = self.params
        T = p.rollout_dict['history_len'] + p.loss_dict['rollout_len']
        shape = (p.train_batch_size, T, p.slot_dict['num_slots'], p.slot_dict['slot_size'])
        g = torch.Generator().manual_seed(self.seed + 1000 * epoch + self.rank)
        for _ in range(self.steps_per_epoch):
            yield {'slots': torch.randn(shape, generator=g).to(self.device)}


class SlotsFileDataModule:
    """Slots of a file written by extract.dump_slots (the reference's slots.pkl, video_based/extract_slots.py:50-62) as
    the vp_vqa task's input, with SyntheticSlotsDataModule's `train_loader(epoch)` contract: {'slots': [B, history_len +
    rollout_len, N, D]}, each a window of one stored video drawn by a generator seeded per (seed, epoch, rank): frames
    t0 + k frame_offset (physion.py's frame_offset; 1 = contiguous), t0 below len - (T - 1) frame_offset."""

    def __init__(self, params, path, split='train', steps_per_epoch=8, device='cuda', seed=1234, frame_offset=1):
        from .extract import load_slots
        assert frame_offset >= 1
        self.params, self.steps_per_epoch, self.device, self.seed = params, steps_per_epoch, device, seed
        self.rank = int(os.environ.get('RANK', 0))
        self.frame_offset = int(frame_offset)
        data = load_slots(path)[split]
        self.T = params.rollout_dict['history_len'] + params.loss_dict['rollout_len']
        self.span = (self.T - 1) * self.frame_offset + 1                            # frames a window reaches over
        self.files = [f for f in sorted(data) if data[f].shape[0] >= self.span]     # shorter videos hold no window
        self.videos = [torch.as_tensor(data[f]).float() for f in self.files]
        assert self.videos, f'{path} [{split}]: no video has {self.span} frames'

    def __len__(self):
        return self.steps_per_epoch

    def windows(self, epoch=0):
        """The (video index, first frame) pairs of an epoch, [steps][B]: what train_loader cuts."""
        g = torch.Generator().manual_seed(self.seed + 1000 * epoch + self.rank)
        out = []
        for _ in range(self.steps_per_epoch):
            vi = torch.randint(len(self.videos), (self.params.train_batch_size,), generator=g).tolist()
            out.append([(v, int(torch.randint(self.videos[v].shape[0] - self.span + 1, (1,), generator=g))) for v in vi])
        return out

    def train_loader(self, epoch=0):
        fo = self.frame_offset
        for step in self.windows(epoch):
            yield {'slots': torch.stack([self.videos[v][t0:t0 + self.span:fo] for v, t0 in step]).to(self.device)}


def physion_label_key(fname, split):
    """The labels-CSV key of a stored video (vp_vqa/datasets/physion.py:316-324): the basename without `.mp4`, for the
    readout subset (every split but 'test') without a trailing `_img`, for the test subset without `-redyellow`."""
    key = os.path.basename(fname)
    if key.endswith('.mp4'):
        key = key[:-4]
    if split != 'test' and key.endswith('_img'):
        key = key[:-4]
    if split == 'test':
        key = key.replace('-redyellow', '')
    return key


def read_physion_labels(labels_csv):
    """{key: 0 | 1} of a Physion labels file (readout_labels.csv / labels.csv): the first column is the key, the column
    `ground truth outcome` the label (physion.py:325-328)."""
    import csv
    with open(labels_csv, newline='') as f:
        rows = list(csv.reader(f))
    if not rows or 'ground truth outcome' not in rows[0]:
        raise ValueError(f"{labels_csv}: no column 'ground truth outcome'")
    col = rows[0].index('ground truth outcome')
    out = {}
    for r in rows[1:]:
        if not r:
            continue
        v = r[col].strip().lower()
        if v in ('true', '1', '1.0'):
            out[r[0]] = 1
        elif v in ('false', '0', '0.0'):
            out[r[0]] = 0
        else:
            raise ValueError(f'{labels_csv}: label {r[col]!r} of {r[0]!r} is neither true nor false')
    return out


class SlotsLabelFileDataModule:
    """Slots of a file written by unroll.rollout_slots_file / extract.dump_slots with the labels of a Physion CSV as the
    readout's input (vp_vqa/datasets/physion.py: PhysionSlotsLabelDataset), with SyntheticSlotsLabelDataModule's
    `train_loader(epoch)` contract: {'slots': [B, video_len, N, D], 'label': [B]}, the videos drawn by a generator
    seeded per (seed, epoch, rank).  A stored video without a label, or shorter than video_len, raises."""

    def __init__(self, params, slots_path, labels_csv, split='train', steps_per_epoch=8, device='cuda', seed=1234):
        from .extract import load_slots
        self.params, self.steps_per_epoch, self.device, self.seed = params, steps_per_epoch, device, seed
        self.rank = int(os.environ.get('RANK', 0))
        self.T = params.video_len
        data = load_slots(slots_path)[split]
        labels = read_physion_labels(labels_csv)
        self.files = sorted(data)
        if not self.files:
            raise ValueError(f'{slots_path} [{split}]: no videos')
        self.videos, self.labels = [], []
        for f in self.files:
            key = physion_label_key(f, split)
            if key not in labels:
                raise KeyError(f'{labels_csv}: no label for {f!r} (key {key!r})')
            if data[f].shape[0] < self.T:
                raise ValueError(f'{slots_path} [{split}]: {f!r} has {data[f].shape[0]} frames, video_len is {self.T}')
            self.videos.append(torch.as_tensor(data[f][:self.T]).float())
            self.labels.append(float(labels[key]))

    def __len__(self):
        return self.steps_per_epoch

    def batches(self, epoch=0):
        """The video indices of an epoch, [steps][B]: what train_loader stacks."""
        g = torch.Generator().manual_seed(self.seed + 1000 * epoch + self.rank)
        return [torch.randint(len(self.videos), (self.params.train_batch_size,), generator=g).tolist()
                for _ in range(self.steps_per_epoch)]

    def train_loader(self, epoch=0):
        for vi in self.batches(epoch):
            yield {'slots': torch.stack([self.videos[v] for v in vi]).to(self.device),
                   'label': torch.tensor([self.labels[v] for v in vi]).to(self.device)}


class SyntheticSlotsLabelDataModule:
    """`build_dataset` stand-in of the VQA readout (vp_vqa/datasets/physion.py: physion_slots_label_readout): seeded
    random slots [B, video_len, N, D] with a 0 / 1 label that follows a planted rule the readout can represent --
    label = 1 iff max_t max_{i<j} (<s_i, a> + <s_j, c>) > thr, with seeded directions a, c and thr the median of that
    score under the slot distribution -- so a fit can be seen to learn."""

    def __init__(self, params, steps_per_epoch=8, device='cuda', seed=1234):
        self.params, self.steps_per_epoch, self.device, self.seed = params, steps_per_epoch, device, seed
        self.rank = int(os.environ.get('RANK', 0))
        rd = params.readout_dict
        self.N, self.D, self.T = rd['num_slots'], rd['slot_size'], params.video_len
        g = torch.Generator().manual_seed(seed)
        self.a = torch.randn(self.D, generator=g) / self.D ** 0.5
        self.c = torch.randn(self.D, generator=g) / self.D ** 0.5
        self.thr = float(self.score(torch.randn((512, self.T, self.N, self.D), generator=g)).median())

    def __len__(self):
        return self.steps_per_epoch

    def score(self, slots):
        """[B, T, N, D] -> [B]: max over frames and ordered pairs i < j of <s_i, a> + <s_j, c>."""
        u, v = slots @ self.a, slots @ self.c                       # [B, T, N]
        pair = u.unsqueeze(3) + v.unsqueeze(2)                      # [B, T, i, j]
        keep = torch.ones(self.N, self.N).triu(1).bool()
        return pair.masked_fill(~keep, float('-inf')).flatten(1).max(1)[0]

    def train_loader(self, epoch=0):
        shape = (self.params.train_batch_size, self.T, self.N, self.D)
        g = torch.Generator().manual_seed(self.seed + 1000 * epoch + self.rank)
        for _ in range(self.steps_per_epoch):
            slots = torch.randn(shape, generator=g)
            label = (self.score(slots) > self.thr).float()
            yield {'slots': slots.to(self.device), 'label': label.to(self.device)}


class Method:
    """fit() = epochs x steps of {forward, weighted loss, backward, (all-reduce), clip+Adam, hook}."""

    def __init__(self, model, datamodule, params, ckp_path=None, local_rank=0, use_ddp=False,
                 use_fp16=False):
        self.model, self.datamodule, self.params = model, datamodule, params
        self.ckp_path, self.local_rank, self.use_ddp = ckp_path, local_rank, use_ddp
        if use_fp16:                      # the reference's --fp16 switch = our bf16 compute path
            model.set_compute_dtype('bf16')
        self.world = torch.distributed.get_world_size() if use_ddp else 1
        self.it = 0
        self.use_graph = os.environ.get('SDMI_GRAPH', '1') != '0'
        self.optimizer = None
        self.history = []
        self.epoch = 0                    # the epoch being trained, counted from 1 (0: before fit)
        self.val_history = []             # (step, log) per validation pass, kept by the default log_fn
        self.log_fn = self._keep_log

    def _keep_log(self, log, step=None):
        self.val_history.append((step, log))

    def _get(self, key, default=None):
        p = self.params
        return p.get(key, default) if hasattr(p, 'get') else getattr(p, key, default)

    # img_based/method.py:235-285 (SA / SADiffusion), video_based/method.py:291-341
    def _configure_optimizers(self):
        p = self.params
        # (the readout config sets no weight_decay: nerv's BaseMethod defaults it to 0)
        assert p.optimizer.lower() in ('adam', 'adamw') and self._get('weight_decay', 0.) == 0., \
            'the path covers Adam without weight decay (every shipped config)'
        total = p.max_epochs * len(self.datamodule)
        clip = self._get('clip_grad', 0) or 0
        clip = clip if clip > 0 else 0.0
        # schedule floor: the diffusion methods anneal to 0 (img_based/method.py:277-283,
        # video_based/method.py:186-194 / 331-339); SA / SAVi / VQ-VAE stage 1 run on the base
        # method's schedule, min_lr = lr / 100 (img_based/method.py:69-85, video_based/method.py:86-96)
        # (vp_vqa/method.py:72-90: the SlotFormer task runs on the base schedule too, min_lr = lr / 100, one group at lr)
        from .models import LDMSlotFormer, SADiffusion, SAViDiffusion
        diffusion = isinstance(self.model, (SADiffusion, SAViDiffusion)) and not isinstance(self.model, LDMSlotFormer)
        return FusedAdam(self.model, lr=p.lr, dec_lr=self._get('dec_lr', p.lr), clip_grad=clip,
                         total_steps=total, warmup_pct=p.warmup_steps_pct,
                         min_lr_ratio=(0.0 if diffusion else 0.01))

    def _loss(self, batch):
        out = self.model(batch)
        losses = self.model.calc_train_loss(batch, out)
        total = None
        for k, v in losses.items():
            w = self._get(f'{k}_w', 1.0)
            total = v * w if total is None else total + v * w
        return total, losses

    def _eager_step(self, batch):
        self.optimizer.zero_grad()
        total, losses = self._loss(batch)
        total.backward()
        if self.world > 1:
            if getattr(self, '_reducer', None) is None:
                self._reducer = parallel.GradReducer(self.model.grad_arena(), self.world, self._get('ddp_grad_dtype'))
            r = self._reducer.reduce_all(4)
            self.optimizer.step(grad_src=r.grad_src, grad_scale=r.grad_scale)
        else:
            self.optimizer.step()
        return total.detach()

    def fit(self, resume_from='', san_check_val_step=0, max_steps=None):
        ckp = None
        if resume_from:
            ckp = torch.load(resume_from, map_location='cpu')
            self.model.load_state_dict(ckp.get('state_dict', ckp))
        self.model.train()
        if self.use_ddp:
            parallel.broadcast_parameters(self.model.arena())
        self.optimizer = self._configure_optimizers()
        if ckp is not None:
            self._restore_training_state(ckp)
        graphed = None
        validating = hasattr(self.datamodule, 'val_loader')
        if validating and san_check_val_step > 0:
            self.validate(san_check_step=san_check_val_step)
        steps_per_epoch = len(self.datamodule)
        first_epoch = self.it // max(1, steps_per_epoch)
        # a mid-epoch checkpoint resumes BEHIND the batches it already consumed: the run then sees the
        # same batch sequence, and executes exactly max_epochs * steps_per_epoch steps in total
        skip = self.it - first_epoch * steps_per_epoch
        for epoch in range(first_epoch, self.params.max_epochs):
            self.epoch = epoch + 1
            for bi, batch in enumerate(self.datamodule.train_loader(epoch)):
                if epoch == first_epoch and bi < skip:
                    continue
                if max_steps is not None and self.it >= max_steps:
                    return self
                if self.use_graph and graphed is None and len(self._loss_names()) == 1:
                    ar = True if self.world > 1 else None      # overlapped gradient all-reduce
                    key = self._loss_names()[0]
                    # (the capture's warm-up passes are rolled back: optim.GraphedTrainStep)
                    graphed = GraphedTrainStep(self.model, self.optimizer, batch, allreduce=ar,
                                               loss_key=key, loss_weight=self._get(f'{key}_w', 1.0),
                                               world=self.world, wire=self._get('ddp_grad_dtype'))
                loss = graphed(batch) if graphed is not None else self._eager_step(batch)
                self.it += 1
                self.history.append(loss)
                self.model._training_step_end(self)
                if max_steps is not None and self.it >= max_steps:
                    return self
            if validating and (self.epoch % (self._get('eval_interval', 1) or 1) == 0 or
                               self.epoch == self.params.max_epochs):
                self.validate()
        return self

    def validate(self, san_check_step=-1, sample=True):
        """One validation pass (SlotBaseMethod.validation_epoch of both reference method.py files, with the
        `_sample_img` / `_sample_video` of the model's method class) -> the logged dict, also sent to
        `self.log_fn(log, step=self.it)`, whose default appends (step, log) to `self.val_history`.

        The model is put in eval mode without gradients.  Every batch of `datamodule.val_loader()` goes through
        `model.calc_eval_loss(batch, model(batch))`; each key is averaged WEIGHTED BY BATCH SIZE into `val/<key>`
        (nerv's own loop is not part of the reference tree: the weighting is this project's decision, so that a short
        last batch counts by its samples), stopping after `san_check_step` batches when that is > 0.  With use_ddp the
        per-key sums and the count are all-reduced in one tensor.  On rank 0, with `sample` and a `datamodule.val_set`,
        the model's samples follow (validate.py): the DPM reconstruction loss at the end of an epoch
        (san_check_step <= 0; for videos also in the last epoch) and the slot-decomposition panels, as uint8 numpy
        arrays -- [H, W, 3] for an image, [T, 3, H, W] for a video, what wandb.Image / wandb.Video take.
        `params.val_sampler_kwargs` (optional, default {}) is forwarded to the sampler calls, e.g. dpm_steps.

        Training is not moved: torch's generator states and the model's training / testing flags are restored, the
        sampler noise comes from a generator seeded by (seed, self.it), and the inference operands are refreshed from
        the weights of the step just taken.  Only the model's eval_seed stream advances."""
        from .validate import run_validation
        return run_validation(self, san_check_step, sample)

    def _loss_names(self):
        from .models import SA, VQVAE
        if getattr(self.model, 'loss_names', None):       # LDMSlotFormer: slot_recon_loss
            return list(self.model.loss_names)
        if isinstance(self.model, VQVAE):        # three weighted terms: eager steps (vqvae/loss.py)
            return ['quant_loss', 'recon_loss', 'percept_loss']
        return ['img_recon_loss'] if isinstance(self.model, SA) else ['denoise_loss']

    def save(self, path):
        """Checkpoint = weights + everything a resumed run needs to continue the same trajectory:
        Adam moments, step (bias correction and schedule position), iteration, EMA shadow."""
        ckp = {'state_dict': self.model.state_dict(), 'it': self.it}
        if self.optimizer is not None:
            ckp['optimizer'] = self.optimizer.state_dict()
        dm = getattr(self.model, 'dm_decoder', None)
        if dm is not None and getattr(dm, 'use_ema', False):
            ckp['ema'] = {'shadow': dm._ema_shadow.detach().cpu(), 'num_updates': dm.ema_num_updates,
                          'decay': dm.ema_decay}
        seed = getattr(self.model, 'step_seed', None)
        if seed is not None:
            ckp['step_seed'] = int(seed)
        eseed = getattr(self.model, 'eval_seed', None)       # validation t / noise draws continue too
        if eseed is not None:
            ckp['eval_seed'] = int(eseed)
        if self.model.arena().is_cuda:           # t / noise draws continue the same stream
            ckp['cuda_rng_state'] = torch.cuda.get_rng_state(self.model.arena().device)
        torch.save(ckp, path)

    def _restore_training_state(self, ckp):
        self.it = int(ckp.get('it', 0))
        if 'optimizer' in ckp:
            self.optimizer.load_state_dict(ckp['optimizer'])
        dm = getattr(self.model, 'dm_decoder', None)
        if dm is not None and 'ema' in ckp:
            e = ckp['ema']
            dm.enable_ema(e['decay'], use_num_updates=e['num_updates'] >= 0)
            dm._ema_shadow.copy_(e['shadow'])
            dm.ema_num_updates = e['num_updates']
        if 'cuda_rng_state' in ckp and self.model.arena().is_cuda:
            torch.cuda.set_rng_state(ckp['cuda_rng_state'], self.model.arena().device)
        if 'step_seed' in ckp:
            dev = self.model.arena().device
            self.model.step_seed = torch.full((1,), ckp['step_seed'], dtype=torch.int64, device=dev)
        if 'eval_seed' in ckp:
            dev = self.model.arena().device
            self.model.eval_seed = torch.full((1,), ckp['eval_seed'], dtype=torch.int64, device=dev)


def build_method(**kwargs):
    """Same call signature as the reference's task.build_method."""
    return Method(**kwargs)
