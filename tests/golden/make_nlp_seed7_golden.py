"""Generates tests/golden/nlp_seed7_{tmp,jit}.npz: what the reference's own generated NLP code (oracle/_ref/libnlp_{tmp,jit}.so,
tmp.c / jit_tmpComMiH.c compiled as is) returns on the three seeded random draws of
tests/test_oracle_nlp.py::test_restatement_matches_compiled_reference, so that test runs without oracle/_ref.

Run where oracle/_ref has been built (oracle/Makefile, needs the reference sources):
    python tests/golden/make_nlp_seed7_golden.py
Stored: the inputs (x, p, lam_f, lam_g), f, g, grad f, jac g and hess L (CCS nnz), nlp_grad's grad_gamma_x / grad_gamma_p, and
the CCS sparsity tables.  These are data (vectors), not reference source.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_nlp  # noqa: E402


def draws(nx=ref_nlp.NX, npar=ref_nlp.NP, ng=ref_nlp.NG):
    """The test's draws, in the test's order."""
    rng = np.random.default_rng(7)
    out = []
    for _ in range(3):
        x, p = rng.normal(size=nx), rng.normal(size=npar)
        lf, lg = rng.normal(), rng.normal(size=ng)
        out.append((x, p, lf, lg))
    return out


def main():
    out_dir = os.path.dirname(os.path.abspath(__file__))
    for which in ("tmp", "jit"):
        ref = ref_nlp.RefNLP(which)
        _, _, jc, jr = ref.sparsity("nlp_jac_fg", "out", 3)
        _, _, hc, hr = ref.sparsity("nlp_hess_l", "out", 0)
        jcol = np.repeat(np.arange(ref_nlp.NX), np.diff(jc))
        hcol = np.repeat(np.arange(ref_nlp.NX), np.diff(hc))
        cols = {k: [] for k in ("x", "p", "lam_f", "lam_g", "f", "g", "grad_f", "jac_nnz", "hess_nnz", "grad_gamma_x", "grad_gamma_p")}
        for x, p, lf, lg in draws():
            f, gf, g, J = ref.jac_fg(x, p)
            H = ref.hess_l(x, p, lf, lg)
            _, _, gx, gp = ref.grad(x, p, lf, lg)
            # RefNLP fills the dense J and H from the CCS nnz alone: the stored nnz describe them fully
            for k, v in zip(cols, (x, p, lf, lg, f, g, gf, J[jr, jcol], H[hr, hcol], gx, gp)):
                cols[k].append(v)
        np.savez_compressed(os.path.join(out_dir, f"nlp_seed7_{which}.npz"), **{k: np.array(v) for k, v in cols.items()},
                            jac_colind=jc, jac_row=jr, hess_colind=hc, hess_row=hr)
        print(which, "written")


if __name__ == "__main__":
    main()
