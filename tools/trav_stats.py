import sys; sys.path.insert(0,'.')
import torch
from icon_amd import synth
from icon_amd.engine import MeshHandle
a = synth.make_assets("body"); T=lambda x: torch.from_numpy(x).cuda()
mesh = MeshHandle(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
# three views of one kernel's counters (k_walk_stats): traversal_stats on pair_box_bound, the other two on the walk the mesh runs
for res in (33, 65, 129, 257):
    print(res, mesh.traversal_stats(res))
    ps = mesh.pair_stats(res)     # the oriented-box cull of the leaf pairs (ICON_AMD_PAIR_BOX=0: off); tools/pair_box_model.py predicts it
    print(res, f"nodes / packet {ps['nodes_per_packet']:.1f}, leaf pairs offered / packet {ps['pairs_offered_per_packet']:.1f}, "
               f"pairs tested / packet {ps['pairs_tested_per_packet']:.1f}")
    ws = mesh.walk_stats(res)     # the same walk: AABB / oriented node visits and leaf visits (ICON_AMD_NODE_BOX=0: AABBs only); tools/node_box_model.py
    n = max(ws["packets"], 1)
    print(res, f"AABB node visits / packet {(ws['nodes'] - ws['oriented_nodes']) / n:.1f}, oriented node visits / packet {ws['oriented_nodes'] / n:.1f}, "
               f"leaf visits / packet {ws['leaves'] / n:.1f}, dependent load rounds / packet {(ws['nodes'] + ws['leaves']) / n:.1f}")
import time
for n in (36000, 100000, 1000000):
    pts = (torch.rand((n, 3), device="cuda") * 2 - 1)
    mesh.sdf_query(pts); torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(5): mesh.sdf_query(pts)
    torch.cuda.synchronize(); print(f"sdf_query {n} random points: {(time.perf_counter()-t)*200:.3f} ms")
