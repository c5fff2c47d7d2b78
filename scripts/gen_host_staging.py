#!/usr/bin/env python3
"""Generates the host-tensor staging layer of the C ABI.

lamp's default device for knnSearch / Umap.umap is CPU (knn/package.scala:145, umap.scala:357) and its gradient suite runs every case
on the CPU first (autograd.test.scala:117-133).  This library computes on the GPU only: an operator that exists only as a kernel,
handed tensors that ALL live in host memory, copies them to the calling thread's current GPU (current stream), runs the very same
kernel, and hands back host tensors - same arithmetic, no second implementation, no oracle.  Mixed host / device arguments still fail
loudly, and operators that do compute on the host (element-wise, reductions, mm, index_select, copies) are untouched.

Mechanism: every C-ABI function DEFINED under csrc/kernels/ is compiled under the name `<name>__dev` (kernels/abi_dev_names.h, force
included by the Makefile for those sources only); core/host_staging.cpp defines the public `<name>`:
    rc = <name>__dev(args);  if (rc != LAMP_STATUS_HOST_TENSOR) return rc;       // 0, or an ordinary error
    all tensor arguments on the host?  stage -> <name>__dev on the copies -> outputs / in-place results back to the host
`LAMP_STATUS_HOST_TENSOR` (2) is what LAMP_API_END returns for lamp::HostTensorError, thrown by check_device_tensor().

Parameter conventions of include/lamp_hip.h the generator relies on (asserted below):
    lamp_tensor** name         one output handle (may be NULL when the name ends in _or_null)
    lamp_tensor* name[K]       K output handles (entries the mask deselects stay NULL)
    const lamp_tensor* name    input (may be NULL)
    lamp_tensor* name          written in place (running statistics, `self`, `out`)
    lamp_tensor* const* name   array of `n` tensors written in place / read (parameter `n` of the same function)

Usage: python scripts/gen_host_staging.py   (writes the two files; tests/test_host_staging.py checks they are current)"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lamp_amd._capi import parse_header  # noqa: E402

CSRC = os.path.join(ROOT, "lamp_amd", "csrc")
OUT_NAMES = os.path.join(CSRC, "kernels", "abi_dev_names.h")
OUT_CPP = os.path.join(CSRC, "core", "host_staging.cpp")


def defined_outside_kernels():
    names = set()
    for sub in ("core", "host"):
        d = os.path.join(CSRC, sub)
        for f in sorted(os.listdir(d)):
            if not f.endswith((".cpp", ".hip")) or f == "host_staging.cpp":
                continue
            src = open(os.path.join(d, f)).read()
            names |= set(re.findall(r'^(?:extern "C" )?(?:int|const char\*) (lamp_\w+)\(', src, flags=re.M))
    return names


def classify(param):
    p = re.sub(r"/\*.*?\*/", "", param).strip()
    m = re.match(r"^(.*?)\b(\w+)(\[(\d*)\])?$", p)
    typ, name, arr = m.group(1).strip().replace(" *", "*"), m.group(2), m.group(4)
    if "lamp_tensor" not in typ:
        return ("plain", name, None)
    if typ == "lamp_tensor**":
        return ("out1", name, None)
    if typ == "lamp_tensor*" and m.group(3):
        return ("outk", name, int(arr))
    if typ == "const lamp_tensor*":
        return ("in", name, None)
    if typ == "lamp_tensor*":
        return ("inout", name, None)
    if typ == "lamp_tensor* const*":
        return ("arr", name, None)
    raise SystemExit(f"gen_host_staging: unknown tensor parameter form {param!r}")


# tensor ARRAYS the operator only reads (everything else `lamp_tensor* const*` may be written in place): staged without a copy back
# (gradients handed to an optimiser step came back re-written into the caller's host tensors after every call)
READ_ONLY_ARRAYS = {("lamp_cat", "ts"), ("lamp_cat_out", "ts"), ("lamp_stack", "ts"), ("lamp_adamw_step_", "grads"), ("lamp_sgdw_step_", "grads"),
                    ("lamp_flatten_into_", "ts"), ("lamp_radam_step_", "grads"),     # NOT lamp_yogi_step_'s: Yogi writes its gradients,
                    ("lamp_symmetric_eig", "matrices"),                              # nor lamp_shampoo_step_'s: momentum blends into them
                    ("lamp_recurrent_decode_pack", "tensors"), ("lamp_swa_average_", "cur"), ("lamp_state_copy_", "src")}


def generate():
    decls = parse_header(os.path.join(ROOT, "include", "lamp_hip.h"))
    for fn, pn in READ_ONLY_ARRAYS:
        assert fn in decls and any(re.search(r"lamp_tensor\* ?const\* ?%s$" % pn, re.sub(r"/\*.*?\*/", "", p).strip()) for p in decls[fn][2]), (fn, pn)
    outside = defined_outside_kernels()
    fns = []
    for name, (_, _, plist) in decls.items():
        if name in outside:
            continue
        kinds = [classify(p) for p in plist]
        if not any(k[0] != "plain" for k in kinds):
            continue                                  # no tensor argument: nothing to stage (creation functions handle device = -1 themselves)
        if any(k[0] == "arr" for k in kinds):
            assert any(k[1] == "n" for k in kinds), f"{name}: tensor array without a count parameter `n`"
        fns.append((name, plist, kinds))
    fns.sort()
    names = ["// GENERATED by scripts/gen_host_staging.py - do not edit.  Force-included (Makefile) into csrc/kernels/*.hip only: the C-ABI functions",
             "// defined there are compiled as <name>__dev; core/host_staging.cpp defines the public names.", "#pragma once"]
    names += [f"#define {n} {n}__dev" for n, _, _ in fns]
    cpp = ['// GENERATED by scripts/gen_host_staging.py - do not edit.  See that script for the design; the mechanism is lamp::staging::call',
           '// (host_staging.h): one line per entry point names the role of every parameter.',
           '#include "host_staging.h"', "", "namespace S = lamp::staging;", "", 'extern "C" {', ""]
    for name, plist, kinds in fns:
        sig = ", ".join(plist)
        roles = []
        for kind, pn, k in kinds:
            if kind == "plain":
                roles.append(pn)
            elif kind == "in":
                roles.append(f"S::In{{{pn}}}")
            elif kind == "inout":
                roles.append(f"S::InOut{{{pn}}}")
            elif kind == "arr":
                ro = "true" if (name, pn) in READ_ONLY_ARRAYS else "false"
                roles.append(f"S::Arr{{{pn}, n, {ro}}}")
            elif kind == "out1":
                roles.append(f"S::Out{{{pn}}}")
            elif kind == "outk":
                roles.append(f"S::OutK<{k}>{{{pn}}}")
        cpp.append(f"int {name}__dev({sig});")
        cpp.append(f"int {name}({sig}) {{ return S::call({name}__dev, {', '.join(roles)}); }}")
    cpp.append('}  // extern "C"')
    return "\n".join(names) + "\n", "\n".join(cpp) + "\n", [f[0] for f in fns]


def main():
    names, cpp, fns = generate()
    open(OUT_NAMES, "w").write(names)
    open(OUT_CPP, "w").write(cpp)
    print(f"wrote {OUT_NAMES} and {OUT_CPP}: {len(fns)} staged entry points")


if __name__ == "__main__":
    main()
