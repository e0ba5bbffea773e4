"""icon_amd - MI355X-native implicit-surface query engine for ICON (gfx950, HIP).

Public surface (mirrors the reference's query interface, see icon_amd/engine.py):
    IconQueryEngine.query      == HGPIFuNet.query        (lib/net/HGPIFuNet.py:268-367)
    query_func                 == lib/common/train_util.py:324-348
    DenseReconEngine           == the reconEngine object (lib/common/seg3d_lossless.py:36)
    training.attach            == HGPIFuNet.query in train mode: native rows of every stack + their gradient (icon_amd/training.py; icon, pifu and pamir)
The compute path is libicon_amd.so (include/icon_amd.h); there is no CPU fallback.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # lazy: `import icon_amd` must not need torch or the shared library
    if name in ("IconQueryEngine", "MeshHandle", "FeatHandle", "MlpHandle", "query_func"):
        from . import engine
        return getattr(engine, name)
    if name in ("DenseReconEngine", "slab_bounds", "export_mesh_numpy"):
        from . import recon
        return getattr(recon, name)
    if name in ("extract_cloth", "extract_cloth_device", "nearest_vertex_device", "transfer_labels_device"):
        from . import garment
        return getattr(garment, name)
    if name in ("ScanMesh", "GeoSampler", "sample_geo_device", "smpl_signs_device"):
        from . import sampling
        return getattr(sampling, name)
    if name in ("point_features_device", "TrainQuery"):
        from . import training
        return getattr(training, name)
    raise AttributeError(name)
