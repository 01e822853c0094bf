"""Elementwise losses given as expressions: ``ExprLoss(tree, options)``.

The reference accepts any Julia function as ``elementwise_loss`` (src/LossFunctions.jl:13-33, the
``loss::Function`` branches of ``_loss`` / ``_weighted_loss``).  A Python callable here runs on the host
over predictions copied from the device; an ``ExprLoss`` is the same loss written as a ``Node`` tree over
``Node(feature=1)`` (prediction), ``Node(feature=2)`` (target) and ``Node(feature=3)`` (weight), which the
device evaluates itself (srhip_eval_loss_expr): the predictions never leave it.

    p, t = srhip.Node(feature=1), srhip.Node(feature=2)
    opts = srhip.Options(binary_operators=("+", "-", "*", "^"), unary_operators=("abs",))
    loss = srhip.ExprLoss(srhip.Node("abs", p - t) ** 2.5, opts)
    srhip.Options(..., elementwise_loss=loss)

Operators are named from ``options``' operator lists and mean what they mean in a tree of the population:
``^`` is safe_pow, ``log`` is safe_log, ``sqrt`` is safe_sqrt (NaN outside their domains), every value in
the dataset's element type.  The options given here only name the loss's operators; they need not be the
search's.  An ``ExprLoss`` is also a callable ``loss(pred, y)`` / ``loss(pred, y, w)`` (the host
interpreter of the same program, srhip_loss_expr_eval_host), so every path that takes a callable loss
takes it.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import check, ptr
from .node import Node, flatten


class ExprLoss:
    def __init__(self, tree: Node, options, nargs: int | None = None):
        self.tree = Node.lift(tree)
        self.options = options
        feats = [n.feature for n in self.tree if n.degree == 0 and not n.constant]
        # l(pred, y) unless the weight is read (a weighted dataset calls l(pred, y, w): pass nargs=3
        # for a loss that takes the weight without reading it)
        self.nargs = int(nargs) if nargs is not None else (3 if any(f == 3 for f in feats) else 2)
        self._handles = {}

    def handle(self, dtype) -> ctypes.c_void_p:
        """The compiled expression for element type dtype (srhip_loss_expr_create, once per type)."""
        dt = np.dtype(dtype)
        h = self._handles.get(dt)
        if h is None:
            nodes, _ = flatten([self.tree], self.options, dt if dt != np.int32 else np.float64)
            ops = self.options.c_operators()
            h = ctypes.c_void_p()
            check(_lib.load().srhip_loss_expr_create(_lib.dtype_code(dt), ptr(nodes), len(nodes), ctypes.byref(ops),
                                                     self.nargs, ctypes.byref(h)))
            self._handles[dt] = h
        return h

    def __call__(self, pred, y, w=None):
        """The per-element loss values in pred's type, computed on the host by the library."""
        p = np.asarray(pred)
        dt = p.dtype if p.dtype in (np.float32, np.float64) else np.dtype(np.float64)
        shape = p.shape
        p = np.ascontiguousarray(p, dtype=dt).reshape(-1)
        yv = np.ascontiguousarray(np.broadcast_to(np.asarray(y, dtype=dt), shape)).reshape(-1)
        if self.nargs == 3 and w is None:
            raise TypeError("this loss takes (pred, y, w)")
        wv = None if w is None else np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=dt), shape)).reshape(-1)
        out = np.empty(p.shape, dtype=dt)
        check(_lib.load().srhip_loss_expr_eval_host(self.handle(dt), ptr(p), ptr(yv), ptr(wv), p.size, ptr(out)))
        return out.reshape(shape) if shape else out[0]

    def instructions(self, dtype):
        """srhip_loss_expr_instructions: (ins, need) of the program compiled for dtype; ins is a list of
        (op, dst, a, b, imm) in execution order, op an operator's device code or 0x100 .. 0x103 for a load of
        the prediction, the target, the weight or a constant (imm: its bits in dtype)."""
        lib = _lib.load()
        h = self.handle(dtype)
        n, need = ctypes.c_int32(), ctypes.c_int32()
        check(lib.srhip_loss_expr_instructions(h, None, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(need)))
        op = np.zeros(n.value, dtype=np.uint32)
        dst, a, b = (np.zeros(n.value, dtype=np.int32) for _ in range(3))
        imm = np.zeros(n.value, dtype=np.uint64)
        check(lib.srhip_loss_expr_instructions(h, ptr(op), ptr(dst), ptr(a), ptr(b), ptr(imm), n.value, ctypes.byref(n),
                                               ctypes.byref(need)))
        return [tuple(int(v[i]) for v in (op, dst, a, b, imm)) for i in range(n.value)], int(need.value)

    def close(self):
        for h in self._handles.values():
            _lib.load().srhip_loss_expr_destroy(h)
        self._handles = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __getstate__(self):  # the C handles are rebuilt on use
        d = dict(self.__dict__)
        d["_handles"] = {}
        return d

    def __repr__(self):
        from .node import string_tree

        return f"ExprLoss({string_tree(self.tree, self.options)})"
