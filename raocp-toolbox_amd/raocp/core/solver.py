# SPDX-License-Identifier: Apache-2.0
# API restated from raocp-toolbox (Apache-2.0, Moran, Zhang, Sopasakis); see NOTICE.
"""Chambolle–Pock solver (reference: raocp/core/solver.py:12-253).

`chock` runs the whole loop on the GPU: step size by device Lanczos on L'L
(replacing ARPACK `eigs`, solver.py:104-118), then `raocp_cp_run`, which
replays the CP iteration as a captured hipGraph (dynamics sweeps, fused
L + prox_g* + xi2 kernel, fused L^T + AVaR-kernel projection + residual kernel,
on-device stopping test) and only syncs with the host every 24 iterations. Like the
reference, a solve continues from the cache's current (old) primal / dual.
Residual histories, return codes and the two timer prints are the reference's.
The host-orchestrated half steps (`primal_k_plus_half` ...) are kept for API
parity; each of their operators is still a HIP kernel.
"""
import time

import numpy as np

import raocp.core.cache as cache
import raocp.core.operators as ops
import raocp.core.raocp_spec as spec

__all__ = ["Solver", "normalise_initial_states", "normalise_scenarios", "sample_scenarios", "normalise_accel",
           "BatchSimulation", "Evaluation"]


def normalise_initial_states(initial_states, nx):
    """The (B, nx) float64 array of a batch's initial states: accepts (B, nx), (B, nx, 1) and,
    for one instance, a 1-D array of nx entries; anything else raises ValueError."""
    a = np.asarray(initial_states, dtype=np.float64)
    if a.ndim == 1 and a.size == nx:
        a = a.reshape(1, nx)
    elif a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim != 2 or a.shape[1] != nx or a.shape[0] < 1:
        raise ValueError(f"initial_states of shape {np.shape(initial_states)}: expected (B, {nx}) or (B, {nx}, 1)")
    return np.ascontiguousarray(a)


def normalise_scenarios(scenarios, B, T, n_children):
    """The (B, T) int32 array of a simulation's realised scenarios (indices into the root's
    children): a wrong shape, a non-integer dtype or an entry outside [0, n_children) raises
    ValueError."""
    a = np.asarray(scenarios)
    if a.shape != (B, T):
        raise ValueError(f"scenarios of shape {a.shape}: expected ({B}, {T})")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"scenarios of dtype {a.dtype}: expected integers")
    if a.size and (a.min() < 0 or a.max() >= n_children):
        raise ValueError(f"scenario entries must be in [0, {n_children}): found {int(a.min())} .. {int(a.max())}")
    return np.ascontiguousarray(a, dtype=np.int32)


def sample_scenarios(probabilities, B, T, seed=None):
    """(B, T) i.i.d. draws of a root child from the children's conditional probabilities with
    np.random.default_rng(seed)."""
    p = np.asarray(probabilities, dtype=np.float64).reshape(-1)
    rng = np.random.default_rng(seed)
    return rng.choice(p.size, size=(B, T), p=p / p.sum()).astype(np.int32)


def normalise_accel(accel, accel_every=1, accel_reg=1e-10, accel_safeguard=1.0):
    """The acceleration options of chock_batch / simulate_batch as the native layer takes them:
    None for accel = 0 (the plain solve), else (m, every, reg, safeguard) with 1 <= m <= 8. An
    accel that is no integer in 0 .. 8, accel_every < 1 or a negative (or NaN) accel_reg /
    accel_safeguard raises ValueError; nothing native is called."""
    if not accel:
        return None
    if not (isinstance(accel, (int, np.integer)) and 1 <= accel <= 8):
        raise ValueError(f"accel must be 0 or in 1 .. 8, got {accel!r}")
    if int(accel_every) < 1 or not accel_reg >= 0.0 or not accel_safeguard >= 0.0:
        raise ValueError("accel_every must be >= 1, accel_reg and accel_safeguard >= 0")
    return int(accel), int(accel_every), float(accel_reg), float(accel_safeguard)


_ACCEL_REFUSED = ("accel > 0 needs the fp64 batch kernel: not available on a float32 solver, "
                  "a sharded context or a context the batch kernel does not cover")


class BatchSimulation:
    """The result of Solver.simulate_batch: states (B, T+1, nx), inputs (B, T, nu),
    stage_costs (B, T), status (B, T), iterations (B, T), errors (B, T, 3) and the realised
    scenarios (B, T). accel_counts is None for a plain simulation; for accel=m it is the (B, T, 4)
    int array of what the acceleration did in each step's solve: proposals made, trials accepted,
    trials rejected, solves refused (zero for the steps a frozen instance did not solve)."""

    def __init__(self, states, inputs, stage_costs, status, iterations, errors, scenarios, accel_counts=None):
        self.states = states
        self.inputs = inputs
        self.stage_costs = stage_costs
        self.status = status
        self.iterations = iterations
        self.errors = errors
        self.scenarios = scenarios
        self.accel_counts = accel_counts


class Evaluation:
    """What a computed policy costs and how far it is from feasible (Solver.evaluate /
    evaluate_batch): cost, the nested-AVaR objective V_0 of the primal's states and inputs;
    epigraph, the primal's own s_0 (equal to the cost only at convergence); box_violation, the
    largest amount by which an active box is missed (0 without boxes); dynamics_residual, the
    largest |x_0 - x0| and |x_j - A_j x_anc(j) - B_j u_anc(j)| entry; node_values, None or the
    (n,) cost-to-go of every node (leaves: the terminal cost). Floats for one solve, (B,) arrays
    for a batch."""

    def __init__(self, cost, epigraph, box_violation, dynamics_residual, node_values=None):
        self.cost = cost
        self.epigraph = epigraph
        self.box_violation = box_violation
        self.dynamics_residual = dynamics_residual
        self.node_values = node_values

    def __repr__(self):
        return (f"Evaluation(cost={self.cost!r}, epigraph={self.epigraph!r}, box_violation={self.box_violation!r}, "
                f"dynamics_residual={self.dynamics_residual!r})")


class Solver:
    def __init__(self, problem_spec: spec.RAOCP, device=None, dtype="float64"):
        self.__raocp = problem_spec
        self.__cache = cache.Cache(self.__raocp, device=device, dtype=dtype)
        self.__operator = ops.Operator(self.__cache)
        self.__initial_state = None
        self.__parameter_1 = None
        self.__parameter_2 = None
        self.__error = [np.zeros(1)] * 3
        self.__delta_error = [np.zeros(1)] * 3
        self.__error_cache = None
        self.__delta_error_cache = None
        self.__batch_size = 0
        self.batch_error_cache = []
        self.batch_delta_error_cache = []
        self.batch_simulation = None
        self.batch_accel_log = []

    @property
    def cache(self):
        return self.__cache

    @property
    def step_size(self):
        return self.__parameter_1

    # ----- host-orchestrated half steps (solver.py:27-61)
    def primal_k_plus_half(self):
        _, template = self.__cache.get_primal()
        _, old_dual = self.__cache.get_dual()
        self.__operator.ell_transpose(old_dual, template)
        _, old_primal = self.__cache.get_primal()
        self.__cache.set_primal([a - self.__parameter_1 * b for a, b in zip(old_primal, template)])

    def primal_k_plus_one(self):
        self.__cache.proximal_of_f(self.__parameter_1)

    def dual_k_plus_half(self):
        _, template = self.__cache.get_dual()
        primal, old_primal = self.__cache.get_primal()
        self.__operator.ell([2 * a - b for a, b in zip(primal, old_primal)], template)
        _, old_dual = self.__cache.get_dual()
        self.__cache.set_dual([a + self.__parameter_2 * b for a, b in zip(old_dual, template)])

    def dual_k_plus_one(self):
        self.__cache.proximal_of_g_conjugate(self.__parameter_2)

    def _calculate_chock_errors(self):
        p_new, p = self.__cache.get_primal()
        d_new, d = self.__cache.get_dual()
        a1, a2 = self.__parameter_1, self.__parameter_2
        d_minus = [x - y for x, y in zip(d, d_new)]
        _, lt = self.__cache.get_primal()
        self.__operator.ell_transpose(d_minus, lt)
        xi_1 = [(x - y) / a1 - z for x, y, z in zip(p, p_new, lt)]
        p_diff = [x - y for x, y in zip(p_new, p)]
        _, lp = self.__cache.get_dual()
        self.__operator.ell(p_diff, lp)
        xi_2 = [x / a2 + y for x, y in zip(d_minus, lp)]
        _, lt2 = self.__cache.get_primal()
        self.__operator.ell_transpose(xi_2, lt2)
        xi_0 = [x + y for x, y in zip(xi_1, lt2)]
        delta_2 = [x - y for x, y in zip(d_new, d)]
        _, lt3 = self.__cache.get_primal()
        self.__operator.ell_transpose(delta_2, lt3)
        delta_0 = [x - y for x, y in zip(p_diff, lt3)]
        return xi_0, xi_1, xi_2, delta_0, p_diff, delta_2

    # ----- the CP loop (solver.py:97-171)
    def compute_step_size(self):
        lam = self.__cache.native.step_size()
        self.__parameter_1 = self.__parameter_2 = 0.999 / lam
        return lam

    def chock(self, initial_state, max_iters=10, tol=1e-5, step_size=None):
        """Chambolle-Pock algorithm. Returns 0 if converged (k < max_iters), else 1.
        `step_size` (extension) pins alpha instead of estimating 0.999/||L||^2."""
        self.__initial_state = initial_state
        self.__cache.cache_initial_state(initial_state)
        if step_size is None:
            self.compute_step_size()
        else:
            self.__parameter_1 = self.__parameter_2 = float(step_size)
        x0 = np.asarray(initial_state, dtype=np.float64).reshape(-1)
        # the loop continues from the cached old primal / dual (x0 in node 0's state), as
        # the reference's does: a second chock warm-starts from the first one's iterate
        self.__cache.seed_device_iterate()
        print("timer started")
        tick = time.perf_counter()
        status, err, derr = self.__cache.native.cp_run(x0, int(max_iters), float(tol), self.__parameter_1,
                                                       warm=True)
        tock = time.perf_counter()
        print(f"timer stopped in {tock - tick:0.4f} seconds")
        self.__error = list(err[-1])
        self.__delta_error = list(derr[-1])
        # one row per iteration; a single iteration leaves a 1-D array (solver.py:148-153)
        self.__error_cache = err if err.shape[0] > 1 else err[0]
        self.__delta_error_cache = derr if derr.shape[0] > 1 else derr[0]
        self.__cache.update_cache()
        return status

    # ----- batched solves (extension): many initial states, one launch
    def chock_batch(self, initial_states, max_iters=10, tol=1e-5, step_size=None, warm=False,
                    accel=0, accel_every=1, accel_reg=1e-10, accel_safeguard=1.0):
        """Chambolle-Pock for B initial states of the same problem at once (one workgroup per
        instance on the device). Returns an int array of chock's codes (0 converged, 1 not).
        warm=True continues every instance from the iterate the previous chock_batch left (the
        batch size must be the same). Results: batch_error_cache[b], batch_delta_error_cache[b],
        batch_primal_flat(b), batch_dual_flat(b), batch_first_inputs(). If a NaN reached a box
        projection in some instances, the results are stored and ValueError names them.
        A float32 solver returns the same types, shapes and dtypes; it runs the batch kernel's
        float form when the environment has RAOCP_CPB_F32=1 and the solves one after another
        otherwise (the same holds for simulate_batch).

        accel=m (1 <= m <= 8) adds Anderson acceleration of memory m. With
        v = (z, eta), g = T(v) one CP iteration and r = g - v, the last m differences of (g, r) are
        kept; after iteration k with (k + 1) % accel_every == 0 the least-squares combination
        gamma = (dR'dR + accel_reg (tr / j) I)^-1 dR'r is solved and g - dG gamma is proposed as
        the next iterate. The iteration after it is a trial: kept if its ||r||_2 is at most
        accel_safeguard times the one before the proposal, else the history is cleared and the
        solve goes on from g. Every iteration, trials included, has its row in the error caches and
        counts against max_iters; a rejected trial never ends the solve through tol.
        batch_accel_log[b] is instance b's (iters, 12) log: code (0 plain, 1 proposal, 2 trial
        accepted, 3 trial rejected, 4 solve refused), column count, what followed (0 nothing, 1 a
        proposal, 2 a refused solve), ||r||_2, gamma[8]. accel=0 (the default) is the plain solve.
        Out of scope: a float32 solver, a sharded context and a context the batch kernel does not
        cover raise ValueError for accel > 0 (there is no sequential fallback); the single-solve
        chock is not accelerated; warm=True after an accelerated batch continues from its iterate
        with an empty history."""
        nx = self.__raocp.state_dynamics_at_node(1).shape[1]
        x0 = normalise_initial_states(initial_states, nx)
        B = x0.shape[0]
        native = self.__cache.native
        aa = normalise_accel(accel, accel_every, accel_reg, accel_safeguard)
        if aa and native.kernel_info(19) == "":
            raise ValueError(_ACCEL_REFUSED)
        z0 = e0 = None
        if warm:
            if B != self.__batch_size:
                raise ValueError(f"warm chock_batch of {B} instances after a batch of {self.__batch_size}")
            pairs = [native.cp_batch_get(b) for b in range(B)]
            z0 = np.array([p[0] for p in pairs])
            e0 = np.array([p[1] for p in pairs])
        if step_size is None:
            self.compute_step_size()
        else:
            self.__parameter_1 = self.__parameter_2 = float(step_size)
        print("timer started")
        tick = time.perf_counter()
        status, errs, derrs = native.cp_batch_run(x0, int(max_iters), float(tol), self.__parameter_1, z0, e0, accel=aa)
        tock = time.perf_counter()
        print(f"timer stopped in {tock - tick:0.4f} seconds")
        self.__batch_size = B
        # the shape rules of error_cache: a single row is 1-D (solver.py:148-153)
        self.batch_error_cache = [e if e.shape[0] > 1 else e[0] for e in errs]
        self.batch_delta_error_cache = [e if e.shape[0] > 1 else e[0] for e in derrs]
        self.batch_accel_log = [native.cp_batch_accel_log(b) for b in range(B)] if aa else []
        bad = [int(b) for b in np.flatnonzero(status == 2)]
        if bad:
            raise ValueError(f"Rectangle constraint - 'nan' value cannot be constrained (instances {bad})")
        return status

    # ----- closed-loop simulation of a batch (extension), resident on the device
    def simulate_batch(self, initial_states, num_steps, scenarios=None, seed=None, max_iters=10, tol=1e-5,
                       step_size=None, warm=True, accel=0, accel_every=1, accel_reg=1e-10, accel_safeguard=1.0):
        """Closed-loop MPC over num_steps steps for B initial states at once: every step solves
        each instance from its current state, applies the root's input and moves the plant along
        the realised scenario (x+ = A_i x + B_i u_0 for the root's child i); warm=True starts each
        solve from the previous step's final iterate. `scenarios` is a (B, num_steps) integer
        array of indices into the root's children; None draws them i.i.d. from the children's
        conditional probabilities with np.random.default_rng(seed). Returns a BatchSimulation
        (also kept as `batch_simulation`); afterwards batch_primal_flat(b), batch_dual_flat(b)
        and batch_first_inputs() describe every instance's last solve. If a NaN reached a box
        projection in some instances, those are frozen from that step on, the results are
        stored and ValueError names them.

        accel=m (1 <= m <= 8) solves every step of every instance with the Anderson-accelerated
        kernel, with the algorithm and the options of chock_batch(accel=m). Every step starts with
        an empty acceleration history whatever `warm` is (a new state is a new fixed-point map);
        warm=True still carries the iterate over. The result's accel_counts is then the (B, T, 4)
        int array of proposals made, trials accepted, trials rejected and solves refused per step,
        and batch_accel_log[b] the log of instance b's last solve. accel=0 (the default) is the
        plain simulation; accel_counts is None. Out of scope: a float32 solver, a sharded context
        and a context the batch kernel does not cover raise ValueError for accel > 0 (there is no
        sequential fallback and no float form)."""
        nx = self.__raocp.state_dynamics_at_node(1).shape[1]
        x0 = normalise_initial_states(initial_states, nx)
        B, T = x0.shape[0], int(num_steps)
        native = self.__cache.native
        aa = normalise_accel(accel, accel_every, accel_reg, accel_safeguard)
        if aa and native.kernel_info(20) == "":
            raise ValueError(_ACCEL_REFUSED)
        tree = self.__raocp.tree
        if scenarios is None:
            scen = sample_scenarios(tree.conditional_probabilities_of_children(0), B, T, seed)
        else:
            scen = normalise_scenarios(scenarios, B, T, len(tree.children_of(0)))
        if step_size is None:
            self.compute_step_size()
        else:
            self.__parameter_1 = self.__parameter_2 = float(step_size)
        print("timer started")
        tick = time.perf_counter()
        counts = None
        if aa:
            X, U, cost, status, iters, err, counts = native.cp_batch_mpc(x0, scen, int(max_iters), float(tol),
                                                                         self.__parameter_1, warm, accel=aa)
        else:
            X, U, cost, status, iters, err = native.cp_batch_mpc(x0, scen, int(max_iters), float(tol),
                                                                 self.__parameter_1, warm)
        tock = time.perf_counter()
        print(f"timer stopped in {tock - tick:0.4f} seconds")
        self.__batch_size = B
        self.batch_simulation = BatchSimulation(X, U, cost, status, iters, err, scen, counts)
        self.batch_accel_log = [native.cp_batch_accel_log(b) for b in range(B)] if aa else []
        bad = [int(b) for b in np.flatnonzero((status == 2).any(axis=1))]
        if bad:
            step = [int(np.argmax(status[b] == 2)) for b in bad]
            raise ValueError(f"Rectangle constraint - 'nan' value cannot be constrained (instances {bad} at steps {step})")
        return self.batch_simulation

    def batch_primal_flat(self, b):
        return self.__cache.native.cp_batch_get(b)[0]

    def batch_dual_flat(self, b):
        return self.__cache.native.cp_batch_get(b)[1]

    def batch_first_inputs(self):
        return self.__cache.native.cp_batch_first_inputs()

    # ----- evaluation of the computed policy (extension)
    def evaluate(self, node_values=False):
        """The Evaluation of the primal the last chock left, against its initial state."""
        res = self.__cache.native.evaluate(None, node_values=node_values)
        out, vals = res if node_values else (res, None)
        return Evaluation(float(out[0]), float(out[1]), float(out[2]), float(out[3]), vals)

    def evaluate_batch(self):
        """The Evaluation of every instance of the last chock_batch or simulate_batch (there: of
        each instance's last solve, as batch_primal_flat describes it); the fields are (B,) arrays."""
        out = self.__cache.native.cp_batch_evaluate()
        return Evaluation(out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy(), out[:, 3].copy())

    # ----- outputs (solver.py:173-253)
    @property
    def error_cache(self):
        return self.__error_cache

    @property
    def delta_error_cache(self):
        return self.__delta_error_cache

    def print_states(self):
        primal, _ = self.__cache.get_primal()
        seg_p = self.__cache.get_primal_segments()
        print("states =\n")
        for i in range(seg_p[1], seg_p[2]):
            print(f"{primal[i]}\n")

    def print_inputs(self):
        primal, _ = self.__cache.get_primal()
        seg_p = self.__cache.get_primal_segments()
        print("inputs =\n")
        for i in range(seg_p[2], seg_p[3]):
            print(f"{primal[i]}\n")

    @staticmethod
    def _tikz_save(name, fallback=None):
        """tikzplotlib.save(name) as the reference does (solver.py:199, 253); tikzplotlib is
        optional (absent in this image): `fallback(name)` then writes the file itself."""
        try:
            import tikzplotlib
        except ImportError:
            if fallback is not None:
                fallback(name)
            return
        tikzplotlib.save(name)

    def _write_residuals_tex(self, name):
        """The pgfplots file tikzplotlib writes for plot_residuals (the layout of the
        reference's published 4-3-residuals.tex): log-y axis, one table per xi series."""
        ec = np.atleast_2d(self.__error_cache)
        colors = [("steelblue31119180", "31,119,180"), ("darkorange25512714", "255,127,14"),
                  ("forestgreen4416044", "44,160,44")]
        pos = ec[np.isfinite(ec) & (ec > 0)]
        lines = ["% pgfplots residual trace (layout of tikzplotlib's output for Solver.plot_residuals)",
                 "\\begin{tikzpicture}", ""]
        lines += [f"\\definecolor{{{c}}}{{RGB}}{{{rgb}}}" for c, rgb in colors]
        lines += ["", "\\begin{axis}[", "legend cell align={left},", "log basis y={10},",
                  "title={Residual values of Chambolle-Pock algorithm iterations},", "xlabel={iteration},",
                  f"xmin={-0.05 * (len(ec) - 1)!r}, xmax={1.05 * (len(ec) - 1)!r},"]
        if pos.size:
            lines.append(f"ymin={float(pos.min()) / 5!r}, ymax={float(pos.max()) * 2!r},")
        lines += ["ylabel={log(residual value)},", "ymode=log", "]"]
        for q, (c, _) in enumerate(colors):
            lines += [f"\\addplot [thick, {c}]", "table {%"]
            lines += [f"{k} {float(v)!r}" for k, v in enumerate(ec[:, q])]
            lines += ["};", f"\\addlegendentry{{xi_{q}}}"]
        lines += ["\\end{axis}", "", "\\end{tikzpicture}", ""]
        with open(name, "w") as f:
            f.write("\n".join(lines))

    @staticmethod
    def read_residuals_tex(name):
        """The three xi series of a residuals .tex file (this class's or tikzplotlib's) as a
        (k, 3) array."""
        series, cur = [], None
        for line in open(name):
            line = line.strip()
            if line.startswith("table {"):
                cur = []
            elif line.startswith("};") and cur is not None:
                series.append(cur)
                cur = None
            elif cur is not None and line:
                cur.append(float(line.split()[1]))
        return np.array(series).T

    def plot_residuals(self, show=True):
        import matplotlib.pyplot as plt
        ec = np.atleast_2d(self.__error_cache)
        for q in range(3):
            plt.semilogy(ec[:, q], linewidth=2, linestyle="solid")
        plt.title("Residual values of Chambolle-Pock algorithm iterations")
        plt.ylabel(r"log(residual value)", fontsize=12)
        plt.xlabel(r"iteration", fontsize=12)
        plt.legend(("xi_0", "xi_1", "xi_2"))
        self._tikz_save('4-3-residuals.tex', self._write_residuals_tex)
        if show:
            plt.show()

    def plot_solution(self, show=True):
        import matplotlib.pyplot as plt
        primal, _ = self.__cache.get_primal()
        seg_p = self.__cache.get_primal_segments()
        x = primal[seg_p[1]: seg_p[2]]
        u = primal[seg_p[2]: seg_p[3]]
        tree = self.__raocp.tree
        last = tree.num_stages - 1
        fig, axs = plt.subplots(2, np.size(x[0]), sharex="all", sharey="row", squeeze=False)
        fig.set_size_inches(15, 8)
        fig.set_dpi(80)

        def path(j, vals, element):
            pts = [[tree.stage_of(j), vals[j][element][0]]]
            while tree.ancestor_of(j) >= 0:
                j = tree.ancestor_of(j)
                pts.append([tree.stage_of(j), vals[j][element][0]])
            return np.array(pts)

        leaves = tree.nodes_at_stage(last)
        for e in range(np.size(x[0])):
            for leaf in leaves:
                pts = path(leaf, x, e)
                axs[0, e].plot(pts[:, 0], pts[:, 1])
            axs[0, e].set_title(f"state element, x_{e}(t)")
        for e in range(np.size(u[0])):
            for leaf in leaves:
                pts = path(tree.ancestor_of(leaf), u, e)
                axs[1, e].plot(pts[:, 0], pts[:, 1])
            axs[1, e].set_title(f"control element, u_{e}(t)")
        for ax in axs.flat:
            ax.set(xlabel='stage, t', ylabel='value')
            ax.label_outer()
        fig.tight_layout()
        self._tikz_save('python-solution.tex')
        if show:
            plt.show()
