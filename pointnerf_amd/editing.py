"""Scene editing: compose parts of trained point clouds into one scene (the reference's ``run/editing.py:189-212``).

A part is cut out of a checkpoint by a boolean index mask and moved by a 4 x 4 rigid transform ``[Rot | Tran]``.  Its points move
with it; what keeps the part looking the way it was trained is a rotation frame per point, ``Rw2c [M,3,3]``, which the aggregator
applies to every world-space direction before the networks see it (offset to the sample, stored point direction, view direction:
DESIGN.md 4.5).  ``compose_parts`` returns exactly what ``model.set_points(..., editing=True)`` takes.

Convention (kept literally from the reference, ``run/editing.py:201``): for a part moved by ``Rot``

    Rw2c = Rot                    if the part's checkpoint has no ``neural_points.Rw2c``
    Rw2c = Rw2c_old @ Rot^T       otherwise ("w2c is reversed against movement")

The two branches are NOT the same rule -- a part without stored frames behaves as if its old frame were ``Rot @ Rot`` -- and a
checkpoint trained with the identity frame renders its moved copy as trained only under the second one.  Store ``neural_points.Rw2c``
(the identity, ``torch.eye(3)``) in a part's state dict to get ``Rot^T``; this helper does not choose for the caller.  A stored
per-point table ``[N,3,3]`` (a part that is itself a composed scene) is cut by the part's mask and multiplied row by row; the reference
cannot express that case.

The reference's own script cannot run on current torch (it seeds the concatenation with a ``[1,0,63]`` embedding and appends 32-wide
ones), so this function is the supported entry.
"""
import torch


def compose_parts(parts):
    """``parts``: iterable of ``(state, inds, mat)`` --
    ``state``  a checkpoint's state dict (keys ``neural_points.xyz [N,3]``, ``.points_embeding [1,N,F]``, ``.points_conf [1,N,1]``,
               ``.points_dir [1,N,3]``, ``.points_color [1,N,3]`` and optionally ``.Rw2c [3,3] | [N,3,3]``),
    ``inds``   a boolean mask ``[N]`` of the points that belong to the part, or None for all of them,
    ``mat``    the part's 4 x 4 transform (rotation ``mat[:3,:3]``, translation ``mat[:3,3]``), or None for the identity.
    Returns ``(xyz [M,3], embedding [1,M,F], color [1,M,3], dir [1,M,3], conf [1,M,1], Rw2c [M,3,3])``, parts in the given order, on the
    device and in the dtype of the first part's ``xyz``."""
    parts = list(parts)
    if not parts:
        raise ValueError("compose_parts: no parts")
    first = parts[0][0]["neural_points.xyz"]
    dev, dt = first.device, first.dtype
    cols = {k: [] for k in ("xyz", "points_embeding", "points_color", "points_dir", "points_conf", "Rw2c")}
    for state, inds, mat in parts:
        get = lambda k: state["neural_points." + k].detach().to(device=dev, dtype=dt)
        xyz = get("xyz")
        n = xyz.shape[0]
        if inds is None:
            sel = torch.ones(n, dtype=torch.bool, device=dev)
        else:
            sel = torch.as_tensor(inds, device=dev)
            if sel.dtype != torch.bool or tuple(sel.shape) != (n,):
                raise ValueError("compose_parts: a part's index mask must be a bool [%d], got %s %s" % (n, sel.dtype, list(sel.shape)))
        mat = torch.eye(4, device=dev, dtype=dt) if mat is None else torch.as_tensor(mat, dtype=dt, device=dev)
        if tuple(mat.shape) != (4, 4):
            raise ValueError("compose_parts: a part's transform must be 4 x 4, got %s" % list(mat.shape))
        rot = mat[:3, :3]
        xyz = xyz[sel]
        m = xyz.shape[0]
        cols["xyz"].append((torch.cat([xyz, torch.ones_like(xyz[:, :1])], dim=-1) @ mat.transpose(0, 1))[:, :3])      # :199
        for k in ("points_embeding", "points_color", "points_dir", "points_conf"):
            if "neural_points." + k not in state:
                raise ValueError("compose_parts: a part's state dict lacks neural_points." + k)
            cols[k].append(get(k)[:, sel, :])
        if "neural_points.Rw2c" not in state:
            rw = rot[None].expand(m, -1, -1)                                                                            # :201, first branch
        else:
            old = get("Rw2c")
            if old.dim() == 3:
                if old.shape[0] != n:
                    raise ValueError("compose_parts: a per-point Rw2c table must have one frame per point (%d), got %s" % (n, list(old.shape)))
                rw = old[sel] @ rot.transpose(0, 1)
            else:
                rw = (old @ rot.transpose(0, 1))[None].expand(m, -1, -1)                                                # :201, second branch
        cols["Rw2c"].append(rw)
    cat = lambda k, d: torch.cat(cols[k], dim=d).contiguous()
    return cat("xyz", 0), cat("points_embeding", 1), cat("points_color", 1), cat("points_dir", 1), cat("points_conf", 1), cat("Rw2c", 0)
