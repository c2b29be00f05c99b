"""(GPU) The kernels a layer enqueues, in order, with their grids: the record that a host-side change left every launch alone.
Runs one training step through the per-layer calls and one through the stack calls for each hidden size 16 / 32 / 64 /
128 and ten flag sets (plain; GraphNorm + both attentions + residual; gated residual; node attention + residual; softmax
attention; edge residual plain and with rezero - the per-layer path both times; GraphNorm alone; no coordinate update)
on one small two-graph batch, and the per-layer step once more with the input coordinates requiring a gradient (the
first layer then takes the general backward pair). Under a kernel trace, once per library and once more under each of
PVS_EGNN_SPLIT_SMALL=1 and PVS_EGNN_SPLIT_WGRADS=1 (profiles/layer_backward_plan.txt):
    PVS_EGNN_LIB=<library> rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/launch_sequence.py
    python tools/launch_sequence.py --parse DIR OUT.txt      # one line per launch: name, grid, workgroup, LDS
Two libraries enqueue the same work when their OUT.txt files are equal (profiles/linear_job_refactor.txt).
`--screening` traces instead one eager step of each screen (ReceptorScreen on the pose-batch builder and on the filter
path, LibraryScreen on the reuse route alone, with struck slots, with contact attention and with cam, cropped, on the
plain route, cropped on leave-out copies and cropped with either map) at a small shape (130-atom receptor, batch of 3)
and one eager FixedShapeScorer step on two complexes of the cli_default golden root: the record that a
change of the screens' host code left every launch alone (profiles/screening_refactor.txt,
profiles/hit_attribution_refactor.txt, profiles/nowait_refactor.txt, profiles/slot_builder_job.txt,
profiles/library_steps_refactor.txt). `--fp64` runs the loop of the default mode with model
and batch in double (hidden 16 / 32 / 64, the per-layer path: there is no fp64 stack), for a change of the binding's
fp64 side (profiles/functional_dtype_refactor.txt)."""
import csv
import glob
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

FLAGS = {
    'plain': dict(),
    'attn_gn': dict(graphnorm=True, node_attention=True, edge_attention=True, residual=True),
    'gated': dict(residual=True, gated_residual=True),
    'natt_res': dict(node_attention=True, residual=True),
    'softmax': dict(edge_attention=True, softmax_attention=True),
    'eres': dict(edge_residual=True),
    'eres_rezero': dict(edge_residual=True, rezero=True, residual=True),
    'gn': dict(graphnorm=True),
    'nocoords': dict(update_coords=False),
}


def parse(trace_dir, out_path):
    files = glob.glob(trace_dir + '/**/*kernel_trace.csv', recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: (int(r.get('Dispatch_Id', 0) or 0), int(r['Start_Timestamp'])))
    with open(out_path, 'w') as out:
        for r in rows:
            grid, wg = ('x'.join(r[f'{what}_{a}'] for a in 'XYZ') for what in ('Grid_Size', 'Workgroup_Size'))
            out.write(f"{r['Kernel_Name']} grid {grid} wg {wg} lds {r.get('LDS_Block_Size', '?')}\n")
    print(out_path, len(rows), 'launches')


def run(fp64=False):
    import torch
    from tests.test_gpu_properties import make_model, random_graph
    g = random_graph(300, 5000, seed=3, n_graphs=2).to('cuda')
    for hidden in (16, 32, 64) if fp64 else (16, 32, 64, 128):
        for kw in FLAGS.values():
            model, _ = make_model(seed=5, k=hidden, num_layers=2, **kw)
            model.train()
            if fp64:
                model.double()
            # ('0x': the per-layer calls with g_x asked of the first layer too)
            for stack in ('0',) if fp64 else ('0', '1', '0x'):
                os.environ['PVS_EGNN_STACK'] = stack[0]
                g.pos = g.pos.detach().requires_grad_(stack == '0x')
                model.optimiser.zero_grad()
                y = model(g).reshape(-1)
                model.get_loss(torch.ones_like(y), y).backward()
                torch.cuda.synchronize()


def run_screening():
    import tempfile
    import torch
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.screening import LibraryScreen, ReceptorScreen
    from pointvs_amd.synthetic import CONFIGS, random_poses, screening_set
    lig, rec, feats = screening_set(seed=6006, n_nodes=470, n_lig=70)
    near = torch.argsort((rec - lig.mean(0)).norm(dim=1))[:130].sort().values      # 130 atoms: three contact-mask words
    rec, lig_feats, rec_feats = rec[near].contiguous().cuda(), feats[:70], feats[70:][near].contiguous()
    torch.manual_seed(3)
    kw = dict(CONFIGS['cfg2']['model'], num_layers=2)
    model = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **kw).eval()
    for n_lig in (12, 70):         # 70 atoms: no pose-batch builder, the ligand edges are filtered from the full graph
        screen = ReceptorScreen(model, rec, torch.cat([lig_feats[:n_lig], rec_feats], 0), n_lig, 3, 7.0)
        screen(random_poses(lig[:n_lig], 3, seed=5, max_shift=3.0).cuda())
        screen.check()
    slots = [(lig_feats[:n].roll(k, 0).contiguous(), random_poses(lig[:n], 1, seed=90 + k, max_shift=3.0)[0])
             for k, n in enumerate((7, 20, 3))]
    screen = LibraryScreen(model, rec, rec_feats, 3, 20, 7.0)
    screen(slots)
    screen.check()
    # the branches of the step that attribution adds: struck slots, the first layer's attention, per-node heads
    torch.manual_seed(4)
    attending = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **dict(kw, edge_attention=True)).eval()
    screen = LibraryScreen(model, rec, rec_feats, 3, 20, 7.0, struck=True)
    screen.load(slots, rec_drop=[-1, 5, 77])()
    screen.check()
    # ... and the cropped step: its own builder layout, every layer on the one full CSR
    for m, extra in ((attending, dict(contact_attention=1)), (model, dict(cam=True)), (model, dict(crop_radius=6.0))):
        screen = LibraryScreen(m, rec, rec_feats, 3, 20, 7.0, **extra)
        screen(slots)
        screen.check()
    # the routes and variants not traced above: the plain route (hidden 16), a crop_parents screen on leave-one-atom-out
    # copies of the three slots, and the masked map reductions of a cropped screen
    torch.manual_seed(5)
    narrow = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **dict(kw, k=16)).eval()
    screen = LibraryScreen(narrow, rec, rec_feats, 3, 20, 7.0)
    screen(slots)
    screen.check()
    from pointvs_amd.screening import leave_out_plan
    sizes = [int(pose.shape[0]) for _, pose in slots]
    packed_pos = torch.cat([pose for _, pose in slots], 0).cuda()
    packed_feats = torch.cat([f for f, _ in slots], 0).cuda().float()
    packed_ptr = torch.tensor([0] + sizes).cumsum(0).to(device='cuda', dtype=torch.int32)
    screen = LibraryScreen(model, rec, rec_feats, 3, 20, 7.0, crop_radius=6.0, crop_parents=True)
    screen.load_leave_out(packed_pos, packed_feats, packed_ptr, leave_out_plan(sizes, 3)[0],
                          torch.zeros(1, dtype=torch.int32, device='cuda'))()
    screen.check()
    screen.check_leave_out()
    for m, extra in ((attending, dict(contact_attention=1)), (model, dict(cam=True))):
        screen = LibraryScreen(m, rec, rec_feats, 3, 20, 7.0, crop_radius=6.0, cropped_maps=True, **extra)
        screen(slots)
        screen.check()
    # the data-root scorer: one eager fixed-shape step on two complexes of the cli_default golden root
    from pointvs_amd.captured_scoring import FixedShapeScorer
    from tests._fixed_shape_cases import generous_capacities
    from tests.test_gpu_fixed_shape_scoring import make_model
    from tests.test_gpu_parquet_dataset import setting
    _, ds = setting('cli_default')
    scorer = FixedShapeScorer(make_model(ds.feature_dim), ds, 2, generous_capacities(ds, [0, 1]), device='cuda')
    scorer([0, 1])
    scorer.check()
    torch.cuda.synchronize()


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--parse':
        parse(sys.argv[2], sys.argv[3])
    elif sys.argv[1:] == ['--screening']:
        run_screening()
    else:
        run(fp64=sys.argv[1:] == ['--fp64'])
