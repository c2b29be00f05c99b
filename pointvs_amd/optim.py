"""`torch.optim.Adam` and `torch.optim.SGD` whose step (and the `clip_grad_value_` the reference runs just before it,
/root/reference/point_vs/models/point_neural_network_base.py:421-422) is ONE kernel launch for all
parameters (`pvs_adam_clip_step` / `pvs_sgd_clip_step`) instead of torch's dozen multi-tensor
launches. Same update rules, same `state_dict` layouts (`step`, `exp_avg`, `exp_avg_sq`; `momentum_buffer`), so
checkpoints stay interchangeable with the reference's optimisers.

Both have a capturable form for hipGraph replay: what a learning-rate scheduler changes from step to step (lr; OneCycleLR
also cycles Adam's beta1 / SGD's momentum) is then read by the kernel from a few doubles in device memory, which
`push_hyperparameters()` writes from the groups' current Python floats (`pvs_hyper_write`)."""
import torch

from . import _lib


class _PointerTables:
    """What the fused optimisers share: the pointer tables of a launch (one row per tensor) travel to the device through a
    small ring of pinned buffers or, under capture, through pinned tables that belong to the capture; the device blocks of
    hyper-parameters of the capturable forms. None of it is optimiser state: `state_dict` stays torch's."""

    _ROW = 5                # int64 columns of a table row
    _NAME = 'optimiser'
    _KEY_FIELDS = ('dev',)  # what of a work item, besides its tensors' addresses, a remembered table depends on

    def _reset_transients(self):
        # pointer tables travel through a small ring of pinned buffers: a slot is only rewritten once
        # the copy that read it has run (the host may be several steps ahead of the device)
        self._ring, self._slot = [], 0
        self._capture_pool, self._capture_next, self._captured_tables = None, 0, []
        self._recent = {}              # (device, the table's rows) -> ring slot that holds that table on the device
        self._hyper = {}               # (group index, device) -> 4 doubles on that device (made with the plan)
        self._fast = None

    def __setstate__(self, state):
        """copy.deepcopy / pickle of an optimiser carry `defaults`, `state` and `param_groups` only (Optimizer.__getstate__):
        the copy starts with its own empty upload ring, no hyper-parameter blocks and no work list."""
        super().__setstate__(state)
        self._reset_transients()

    def reserve_capture_tables(self, k):
        """Pinned pointer tables for `k` more captured steps (pinned memory cannot be allocated while a capture is open,
        and a captured upload must keep its source for as long as the graph is replayed)."""
        rows = max(64, sum(len(g['params']) for g in self.param_groups))
        left = 0 if self._capture_pool is None else self._capture_pool.shape[0] - self._capture_next
        if left < k:
            self._capture_pool = torch.empty((k, rows, self._ROW), dtype=torch.int64).pin_memory()   # (tables handed out
            self._capture_next = 0                                                    # stay alive in _captured_tables)

    def zero_grad(self, set_to_none=True):
        """torch's zero_grad walks hooks, profiler ranges and foreach groups (~100 us on the host for 34 parameters);
        with set_to_none this is all it does."""
        if not set_to_none:
            return super().zero_grad(set_to_none=False)
        for group in self.param_groups:
            for p in group['params']:
                p.grad = None

    def _group_capturable(self, group):
        return bool(group.get('capturable'))

    def _hyper_block(self, gi, dev):
        """The device block of group `gi` on `dev` (allocated when the plan is made: never under capture)."""
        block = self._hyper.get((gi, dev))
        if block is None:
            block = self._hyper[(gi, dev)] = torch.zeros(4, dtype=torch.float64, device=dev)
        return block

    def push_hyperparameters(self):
        """Writes every capturable group's CURRENT hyper-parameters (Python floats: schedulers keep writing them into
        `param_groups` as ever) into its device block, on the current stream, with the values as kernel arguments: no
        staging buffer, nothing to wait for. step() does this itself unless it is being captured - a capture must not
        contain the write, it would replay the captured values - so whoever replays a captured step calls this before
        the capture and before every replay."""
        if not self._hyper:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'{self._NAME}.push_hyperparameters() inside a capture: the write would be replayed with '
                               f'the captured values - call it before the capture and before every replay')
        lib = _lib.lib()
        for (gi, dev), block in self._hyper.items():
            group = self.param_groups[gi]
            if not self._group_capturable(group) or isinstance(group['lr'], torch.Tensor):
                continue
            vals = self._hyper_values(group)
            _lib.check(lib.pvs_hyper_write(block.data_ptr(), len(vals), *vals, *([0.0] * (4 - len(vals))), _lib.stream(dev)),
                       'pvs_hyper_write')

    def _clip_and_torch_step(self, clip_value):
        """What the kernels do not cover: clip_grad_value_ + torch's own step."""
        self._fast = None
        if clip_value is not None:
            torch.nn.utils.clip_grad_value_([p for g in self.param_groups for p in g['params']], clip_value)
        super().step()

    def _table(self, key, rows, n, dev, capturing):
        """The device table of this launch: `rows()` lists its n rows when they have to be uploaded."""
        if not self._ring or self._ring[0][0].shape[0] < n:
            cap = max(n, 64)
            self._ring = [[torch.empty((cap, self._ROW), dtype=torch.int64).pin_memory(),
                           torch.empty((cap, self._ROW), dtype=torch.int64, device=dev), None] for _ in range(8)]
            self._recent = {}
        hit = None if capturing else self._recent.get(key)
        if hit is not None:
            # addresses seen before (the caching allocator hands the gradients the same few sets of blocks,
            # alternating from step to step): that table is still on the device - no upload, and nothing about
            # these very tensors has to be checked or listed again
            return self._ring[hit][1]
        if capturing:
            # a captured upload is replayed from its pinned source: that buffer belongs to the capture and is
            # never rewritten (a ring slot would be, by the next eager step)
            if self._capture_pool is None or self._capture_next >= self._capture_pool.shape[0]:
                raise RuntimeError(f'{self._NAME}: no pinned table left for this capture - call '
                                   'reserve_capture_tables(k) (or run one eager capturable step) before capturing')
            table_host = self._capture_pool[self._capture_next]
            self._capture_next += 1
            table_host[:n] = torch.tensor(rows(), dtype=torch.int64)
            table_dev = torch.empty((n, self._ROW), dtype=torch.int64, device=dev)
            table_dev.copy_(table_host[:n], non_blocking=True)
            self._captured_tables.append((table_host, table_dev))
            return table_dev
        idx = self._slot
        slot = self._ring[idx]
        self._slot = (self._slot + 1) % len(self._ring)
        if slot[2] is not None:
            slot[2].synchronize()
        # (the slot's previous table is forgotten before it is overwritten)
        self._recent = {k: v for k, v in self._recent.items() if v != idx}
        table_host, table_dev = slot[0], slot[1]
        table_host[:n] = torch.tensor(rows(), dtype=torch.int64)
        table_dev[:n].copy_(table_host[:n], non_blocking=True)
        slot[2] = torch.cuda.Event()
        slot[2].record(torch.cuda.current_stream(dev))
        self._recent[key] = idx
        return table_dev

    def _fused_work(self, closure, clip_value):
        """The opening of step(): runs the closure, refreshes the plan and returns (loss, the plan, an iterator over the
        address keys of its work items in order, whether the stream is being captured) - or (loss, None, None, None) when
        the kernel does not cover this step, and then `_clip_and_torch_step` HAS RUN: the caller only returns the loss.
        Host time counts (small batches are bound by it: tools/host_profile.py): the work list - which parameters have
        gradients, their state tensors, the fusability verdict - is kept from step to step and re-derived only when the
        set of parameters with gradients (or `_signature()`: the groups' flavour, or the state) changes; a pointer table
        already on the device is found again by the (parameter, gradient) addresses alone."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        live = [p.grad is not None for group in self.param_groups for p in group['params']]
        fast = self._fast
        if fast is None or fast['live'] != live or fast['sig'] != self._signature():
            fast = self._plan(live)
        keys = self._address_keys(fast) if fast['fusable'] else None
        # tensors at addresses not seen before are looked at (device, layout, sparsity) BEFORE anything is launched
        if keys is None or any(self._recent.get(key) is None and not self._tensors_fusable(work)
                               for work, key in zip([work for works in fast['groups'] for work in works], keys)):
            self._clip_and_torch_step(clip_value)
            return loss, None, None, None
        capturing = torch.cuda.is_current_stream_capturing()
        # (any capture skips the push - also that of a FusedClipSGD whose `capturable` was cleared after its blocks had been
        # made: not a supported use; its step() used to raise from push_hyperparameters() there)
        if self._hyper and not capturing:
            self.push_hyperparameters()        # (a captured step reads what its caller pushes before each replay)
        return loss, fast, iter(keys), capturing

    def _address_keys(self, fast):
        """Per work item the tuple of its `_KEY_FIELDS` and the (parameter, gradient) addresses of this step - what the
        pointer table on the device is remembered by - or None when the fused kernel must not run: a group option it
        does not cover switched on mid-run (`_groups_fusable`: amsgrad, maximize, ... or a tensor learning rate), or a
        parameter / gradient that is not fp32 any more (`model.half()` / `.double()` after the first step: the kernel
        takes raw pointers as fp32 device memory). What else can change under an unchanged plan (device, layout,
        sparsity) is checked by `_tensors_fusable` whenever the addresses are new; tensors at addresses seen before ARE
        the tensors that passed it."""
        if not self._groups_fusable():
            return None
        f32 = torch.float32
        keys = []
        for works in fast['groups']:
            for work in works:
                key = [work[field] for field in self._KEY_FIELDS]
                for p in work['params']:
                    g = p.grad
                    if p.dtype is not f32 or g.dtype is not f32:
                        return None
                    key.append(p.data_ptr())
                    key.append(g.data_ptr())
                keys.append(tuple(key))
        return keys

    @staticmethod
    def _tensors_fusable(work):
        for p in work['params']:
            g = p.grad
            if (not p.is_cuda or not g.is_cuda or g.is_sparse or g.layout is not torch.strided
                    or not g.is_contiguous() or not p.is_contiguous()):
                return False
        return True


class FusedClipAdam(_PointerTables, torch.optim.Adam):
    """Drop-in `torch.optim.Adam`; `step(clip_value=c)` first clamps every gradient to [-c, c] in
    place. Falls back to torch's own implementation whenever a feature the kernel does not cover is
    on (amsgrad, maximize, differentiable, a tensor learning rate, non-CUDA / non-fp32 parameters).
    `capturable=True` (round 5) keeps the step counters on the device exactly as torch's capturable Adam does (same
    `state_dict`), advances them with one foreach launch and lets the kernel form the bias corrections from them, and
    from the lr and betas that `push_hyperparameters()` wrote to the device (`pvs_adam_clip_step_hyper`): the step
    itself is then two launches that a hipGraph can replay, under a scheduler too."""

    _NAME = 'FusedClipAdam'

    def __init__(self, params, **kwargs):
        super().__init__(params, **kwargs)
        self._reset_transients()

    @staticmethod
    def _hyper_values(group):
        return (float(group['lr']), float(group['betas'][0]), float(group['betas'][1]))

    def _groups_fusable(self):
        for group in self.param_groups:
            if group.get('amsgrad') or group.get('maximize') \
                    or group.get('differentiable') or group.get('decoupled_weight_decay') \
                    or isinstance(group['lr'], torch.Tensor):
                return False
        return True

    def _signature(self):
        return [bool(g.get('capturable')) for g in self.param_groups]

    def _fusable(self):
        if not self._groups_fusable():
            return False
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is not None and (not p.is_cuda or p.dtype != torch.float32 or p.grad.is_sparse
                                           or not p.is_contiguous() or not p.grad.is_contiguous()):
                    return False
        return True

    def load_state_dict(self, state_dict):
        """torch's own, then the step counters where THIS optimiser keeps them: on the host for a non-capturable group
        (a checkpoint read with `map_location=<device>` - as the reference's load_weights reads it,
        point_neural_network_base.py:532 - brings them in as device tensors, torch keeps them there, and torch's Adam
        then reads one counter per parameter back to the host every step; the fused step would refuse the state and fall
        back to exactly that), on the device as fp32 for a capturable one."""
        self._fast = None              # new state tensors, other step counts
        out = super().load_state_dict(state_dict)
        _place_step_counters(self)
        return out

    @torch.no_grad()
    def step(self, closure=None, clip_value=None):
        # (the step counters - one 0-dim CPU tensor per parameter: torch's state_dict layout - are views of one tensor and
        # advance with one add_: `_plan`)
        loss, fast, keys, stream_capturing = self._fused_work(closure, clip_value)
        if fast is None:
            return loss
        lib = _lib.lib()
        for gi, (group, works) in enumerate(zip(self.param_groups, fast['groups'])):
            beta1, beta2 = group['betas']
            for work in works:            # one launch per distinct step count (one, unless the gradient set changed mid-run)
                key = next(keys)
                if work['steps_base'] is not None:
                    work['steps_base'].add_(1)               # (host counters: every parameter's `step` is a view of this tensor)
                else:
                    torch._foreach_add_(work['steps'], 1)    # (capturable: one device launch)
                work['step'] += 1
                step, n, dev = work['step'], work['n'], work['dev']
                capturing = work['on_device'] and stream_capturing
                if work['on_device'] and not capturing and self._capture_pool is None:
                    self.reserve_capture_tables(8)
                table_dev = self._table(key, lambda: [[p.data_ptr(), p.grad.data_ptr(), ea.data_ptr(), es.data_ptr(), p.numel()]
                                                      for p, ea, es in work['items']], n, dev, capturing)
                if work['on_device']:
                    _lib.check(lib.pvs_adam_clip_step_hyper(
                        _lib.ptr(table_dev), n, work['hyper'].data_ptr(),
                        float(group['eps']), float(group['weight_decay']), work['steps'][0].data_ptr(),
                        float(clip_value) if clip_value is not None else 0.0,
                        _lib.stream(dev)), 'pvs_adam_clip_step_hyper')
                else:
                    _lib.check(lib.pvs_adam_clip_step(
                        _lib.ptr(table_dev), n, float(group['lr']), float(beta1), float(beta2),
                        float(group['eps']), float(group['weight_decay']), 1.0 - beta1 ** step, 1.0 - beta2 ** step,
                        float(clip_value) if clip_value is not None else 0.0,
                        _lib.stream(dev)), 'pvs_adam_clip_step')
                # the kernel wrote through raw pointers: tell autograd (and anything that caches by
                # version, e.g. ReceptorScreen) that the parameters changed, as an in-place op would
                torch.autograd.graph.increment_version(work['params'])
        return loss

    def _plan(self, live):
        """The work list of step(): per group, per distinct step count, the parameters with gradients and their state
        (created as torch.optim.Adam._init_group does, non-capturable flavour)."""
        groups, fusable = [], self._fusable()
        self._recent = {}      # (remembered tables hold the OLD plan's state-tensor addresses: exp_avg / exp_avg_sq are not in the key)
        if not fusable:       # (torch's own step creates whatever state its flavour - capturable, amsgrad ... - needs)
            self._fast = {'live': live, 'sig': self._signature(), 'groups': [], 'fusable': False}
            return self._fast
        for gi, group in enumerate(self.param_groups):
            by_step = {}
            for p in group['params']:
                if p.grad is None:
                    continue
                state = self.state[p]
                capturable = bool(group.get('capturable'))
                if len(state) == 0:
                    state['step'] = (torch.zeros((), dtype=torch.float32, device=p.device) if capturable
                                     else torch.tensor(0.0, dtype=torch.float32))
                    state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if (not isinstance(state['step'], torch.Tensor) or state['step'].dtype != torch.float32
                        or state['step'].is_cuda != capturable):
                    fusable = False        # (a state the other flavour left behind: torch's own step sorts it out)
                    continue
                # (capturable: one host read per parameter when the plan is made - never under capture, the plan exists
                # from the eager steps before it)
                by_step.setdefault((float(state['step']), capturable), []).append((p, state))
            works = []
            for (count, on_device), members in by_step.items():
                base = None
                if not on_device:
                    # host counters: torch's state_dict layout wants one 0-dim fp32 tensor per parameter; they become
                    # views of ONE tensor, so that a single add_ advances them all (78 counters of a 6-layer model cost
                    # 0.1 ms per step through _foreach_add_: CPU tensors take its slow path)
                    base = torch.full((len(members),), float(count), dtype=torch.float32)
                    for k, (_, st) in enumerate(members):
                        st['step'] = base[k]
                works.append({'items': [(p, st['exp_avg'], st['exp_avg_sq']) for p, st in members],
                              'steps': [st['step'] for _, st in members], 'step': int(count), 'n': len(members),
                              'dev': members[0][0].device, 'params': [p for p, _ in members], 'on_device': on_device,
                              'steps_base': base,
                              'hyper': self._hyper_block(gi, members[0][0].device) if on_device else None})
            groups.append(works)
        self._fast = {'live': live, 'sig': self._signature(), 'groups': groups, 'fusable': fusable}
        return self._fast


class FusedClipSGD(_PointerTables, torch.optim.SGD):
    """Drop-in `torch.optim.SGD`; `step(clip_value=c)` first clamps every gradient to [-c, c] in place, and clip + step
    are ONE launch for all parameters (`pvs_sgd_clip_step`): momentum, Nesterov, L2 weight decay - what the reference
    constructs (point_neural_network_base.py: momentum 0.9, nesterov). The state is torch's (`momentum_buffer`). Falls back
    to `clip_grad_value_` + torch's own step for whatever the kernel does not cover: CPU or non-fp32 parameters, sparse
    gradients, maximize, dampening, a tensor learning rate or weight decay, differentiable, torch's `fused` flavour or a
    gradient scaler's `grad_scale` / `found_inf`.
    `capturable=True`: lr and momentum are read by the kernel from the device (`pvs_sgd_clip_step_hyper`, written by
    `push_hyperparameters()`), so that a hipGraph of the step can be replayed under a scheduler. The switch is an
    attribute of the optimiser, not a group option: `param_groups` and `state_dict()` stay torch's SGD's."""

    _ROW = 4
    _NAME = 'FusedClipSGD'
    _KEY_FIELDS = ('dev', 'first')

    def __init__(self, params, capturable=False, **kwargs):
        super().__init__(params, **kwargs)
        self.capturable = bool(capturable)
        self._reset_transients()

    def __getstate__(self):
        state = super().__getstate__()
        state['capturable'] = self.capturable
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.capturable = bool(self.__dict__.get('capturable', False))

    def load_state_dict(self, state_dict):
        self._fast = None              # new momentum buffers
        return super().load_state_dict(state_dict)

    def _group_capturable(self, group):
        return self.capturable

    @staticmethod
    def _hyper_values(group):
        return (float(group['lr']), float(group['momentum']))

    def _groups_fusable(self):
        if getattr(self, 'grad_scale', None) is not None or getattr(self, 'found_inf', None) is not None:
            return False
        for group in self.param_groups:
            if group.get('maximize') or group.get('differentiable') or group.get('fused') or group['dampening'] != 0 \
                    or isinstance(group['lr'], torch.Tensor) or isinstance(group['weight_decay'], torch.Tensor) \
                    or (group['nesterov'] and group['momentum'] <= 0):
                return False
        return True

    def _signature(self):
        return [(self.capturable, group['momentum'] != 0) for group in self.param_groups]

    @torch.no_grad()
    def step(self, closure=None, clip_value=None):
        loss, fast, keys, capturing = self._fused_work(closure, clip_value)
        if fast is None:
            return loss
        lib = _lib.lib()
        capturing = self.capturable and capturing
        clip = float(clip_value) if clip_value is not None else 0.0
        replan = False
        for group, works in zip(self.param_groups, fast['groups']):
            for work in works:            # one launch, or two while some parameters have no momentum history yet
                key = next(keys)
                n, dev = work['n'], work['dev']
                if work['first'] and capturing:
                    raise RuntimeError('FusedClipSGD: a parameter takes its first step inside a capture (its momentum '
                                       'buffer does not exist yet) - run one eager step before capturing')
                if self.capturable and not capturing and self._capture_pool is None:
                    self.reserve_capture_tables(8)
                table_dev = self._table(key, lambda: [[p.data_ptr(), p.grad.data_ptr(), 0 if buf is None else buf.data_ptr(),
                                                       p.numel()] for p, buf in work['items']], n, dev, capturing)
                if work['hyper'] is not None and not work['first']:
                    _lib.check(lib.pvs_sgd_clip_step_hyper(
                        _lib.ptr(table_dev), n, work['hyper'].data_ptr(), float(group['weight_decay']),
                        int(bool(group['nesterov'])), clip, _lib.stream(dev)), 'pvs_sgd_clip_step_hyper')
                else:
                    _lib.check(lib.pvs_sgd_clip_step(
                        _lib.ptr(table_dev), n, float(group['lr']), float(group['momentum']), float(group['weight_decay']),
                        int(bool(group['nesterov'])), int(work['first']), clip, _lib.stream(dev)), 'pvs_sgd_clip_step')
                if work['first']:          # the launch filled the new buffers: they are state from here on
                    for p, buf in work['items']:
                        self.state[p]['momentum_buffer'] = buf
                    replan = True
                # the kernel wrote through raw pointers: tell autograd (and anything that caches by
                # version, e.g. ReceptorScreen) that the parameters changed, as an in-place op would
                torch.autograd.graph.increment_version(work['params'])
        if replan:
            self._fast = None
        return loss

    def _plan(self, live):
        """The work list of step(): per group the parameters with gradients, those that have a momentum buffer apart
        from those that get one in this step (`first`: torch clones the gradient into it)."""
        groups, fusable = [], self._groups_fusable()
        self._recent = {}      # (remembered tables hold the OLD plan's buffer addresses: they are not in the key)
        for gi, group in enumerate(self.param_groups):
            works = []
            if fusable:
                with_momentum = group['momentum'] != 0
                old, new = [], []
                for p in group['params']:
                    if p.grad is None:
                        continue
                    if p.dtype != torch.float32 or not p.is_cuda:
                        fusable = False
                        break
                    buf = self.state[p].get('momentum_buffer') if with_momentum else None
                    if with_momentum and buf is None:
                        new.append((p, torch.empty_like(p, memory_format=torch.preserve_format)))
                    elif buf is not None and (buf.dtype != torch.float32 or buf.device != p.device
                                              or not buf.is_contiguous()):
                        fusable = False
                        break
                    else:
                        old.append((p, buf))
                for first, members in ((False, old), (True, new)):
                    if members and fusable:
                        dev = members[0][0].device
                        works.append({'items': members, 'params': [p for p, _ in members], 'n': len(members), 'dev': dev,
                                      'first': first, 'hyper': self._hyper_block(gi, dev) if self.capturable else None})
            groups.append(works)
        self._fast = {'live': live, 'sig': self._signature(), 'groups': groups if fusable else [], 'fusable': fusable}
        return self._fast


def _place_step_counters(optimiser):
    """Adam's step counters where each group's `capturable` flag wants them: on the parameter's device for a capturable
    group, as torch's capturable Adam keeps them, else on the host; fp32 either way."""
    for group in optimiser.param_groups:
        capturable = bool(group.get('capturable'))
        for p in group['params']:
            st = optimiser.state.get(p)
            if st and torch.is_tensor(st.get('step')) and (st['step'].is_cuda != capturable
                                                           or st['step'].dtype != torch.float32):
                st['step'] = st['step'].detach().to(device=p.device if capturable else 'cpu', dtype=torch.float32)


class capturable_window:
    """`with capturable_window(optimiser, n_captures):` - FusedClipAdam, FusedClipSGD or plain torch.optim.Adam in its
    capturable form for the duration, with pinned pointer tables for `n_captures` captured steps. SGD: its `capturable`
    attribute (no group option, no state). Adam: every group's `capturable` option, and the step counters on the device
    as fp32, as torch's capturable Adam keeps them (FusedClipAdam then forms the bias corrections in its kernel). The
    work list is dropped either way. On exit - also when the body raised - flags and counters are as they were."""

    def __init__(self, optimiser, n_captures):
        self.optimiser, self.n_captures = optimiser, n_captures
        self._sgd = isinstance(optimiser, FusedClipSGD)

    def _set(self, form):
        """form: SGD's attribute, or Adam's option group by group."""
        if self._sgd:
            self.optimiser.capturable = form
        else:
            for group, flag in zip(self.optimiser.param_groups, form):
                group['capturable'] = flag
            _place_step_counters(self.optimiser)
        self.optimiser._fast = None

    def __enter__(self):
        self._was = (self.optimiser.capturable if self._sgd else
                     [group.get('capturable', False) for group in self.optimiser.param_groups])
        self._set(True if self._sgd else [True] * len(self._was))
        if hasattr(self.optimiser, 'reserve_capture_tables'):
            self.optimiser.reserve_capture_tables(self.n_captures)
        return self

    def __exit__(self, *exc):
        self._set(self._was)

    def checkpoint_state_dict(self):
        """`optimiser.state_dict()` in the form the optimiser has OUTSIDE the window: a checkpoint written inside it
        would otherwise carry capturable groups with device counters (a resumed run would silently be capturable -
        another FusedClipAdam path, and torch's Adam asserts on CPU parameters). The groups get their own flags back
        and the counters go to the host, as the reference's checkpoints hold them (:501-517)."""
        sd = self.optimiser.state_dict()      # (its groups and its index -> state map are new dicts, the states the live ones)
        for group, flag in zip(sd['param_groups'], [] if self._sgd else self._was):
            group['capturable'] = flag
            for idx in () if flag else group['params']:
                st = sd['state'].get(idx)
                if st is not None and torch.is_tensor(st.get('step')) and st['step'].is_cuda:
                    sd['state'][idx] = dict(st, step=st['step'].detach().cpu())
        return sd
