"""Host reference of the actuated and SOTL controllers -- TEST INFRASTRUCTURE ONLY, plain Python loops (no GPU, no library, nothing of
trainer.py): the two rules of INTEGRATION.md "Baseline controllers", vehicle by vehicle over a state (VecTrafficEnv.get_state /
ms.snapshot) and the tables of Scenario.actuated_tables, with the branch every agent took.  The GPU tests compare the device with it;
tests/test_actuated_host.py compares trainer.actuated_actions / trainer.sotl_actions with it and counts, on the oracle alone, the
branches the GPU cases reach.  Nothing here has a tolerance: integers, and one float32 subtraction and compare per vehicle."""
import numpy as np

GAP_BRANCHES = ('min_green', 'extension', 'forced', 'gap_out', 'skip', 'no_demand')
SOTL_BRANCHES = ('min_green', 'platoon', 'change', 'below')
GAP = dict(min_green=2, max_green=6, gap_sec=3.0)             # the parameters of the closed-loop cases
SOTL = dict(min_green=2, theta=20, mu=2, omega_m=25.0)


def tables(scn, rule, params):
    return scn.actuated_tables(rule, gap_sec=params.get('gap_sec'), omega_m=params.get('omega_m'))


def initial_state(scn, E, min_green):
    """(cur, age, kappa) of a freshly armed or reset handle: the first decision is free."""
    A, PMAX = scn.n_agent, int(scn.green_tab.shape[1])
    return np.zeros((E, A), np.int32), np.full((E, A), min_green, np.int32), np.zeros((E, A, PMAX), np.int32)


def movement_counts(scn, tb, st):
    """cnt and near per movement, vehicle by vehicle."""
    cnt, near = [0] * len(tb['mov']), [0] * len(tb['mov'])
    for l in range(scn.n_lane):
        for k in range(int(st['n'][l])):
            i = int(tb['lane_route_mov'][l, st['r'][l, k]])
            if i < 0:
                continue
            cnt[i] += 1
            if np.float32(np.float32(scn.lane_len[l]) - np.float32(st['x'][l, k])) <= np.float32(tb['zone'][l]):
                near[i] += 1
    return cnt, near


def phase_sums(scn, tb, st, cur):
    """call, dem, red(p | cur[a]) as int lists [A][PMAX] (padded phases 0)."""
    cnt, near = movement_counts(scn, tb, st)
    A, PMAX = tb['n_served'].shape
    call, dem, red = ([[0] * PMAX for _ in range(A)] for _ in range(3))
    for a in range(A):
        for p in range(int(scn.agent_nphase[a])):
            for i in tb['served'][a, p, :tb['n_served'][a, p]]:
                call[a][p] += near[i]
                dem[a][p] += cnt[i]
                if not (int(tb['phase_mask'][i]) >> int(cur[a])) & 1:
                    red[a][p] += cnt[i]
    return call, dem, red


def gap_step(scn, tb, st, cur, age, min_green, max_green, **_):
    """One call of the gap rule for one instance: cur, age int [A] are updated in place.  -> (counts int32 [A, PMAX, 2] = {call, dem},
    the branches taken: a list of names per agent -- a change is 'forced' or 'gap_out', and 'skip' too when it passes a phase)."""
    g, G = min_green, max_green
    call, dem, _ = phase_sums(scn, tb, st, cur)
    took = []
    for a in range(scn.n_agent):
        n, c = int(scn.agent_nphase[a]), int(cur[a])
        if age[a] < g:
            age[a] += 1
            took.append(['min_green'])
        elif age[a] < G and call[a][c] > 0:
            age[a] += 1
            took.append(['extension'])
        else:
            q = None
            for d in range(1, n):
                p = (c + d) % n
                if dem[a][p] > 0:
                    q = p
                    break
            if q is None:
                age[a] = min(age[a] + 1, G)
                took.append(['no_demand'])
            else:
                took.append(['forced' if call[a][c] > 0 else 'gap_out'] + ['skip'] * (q != (c + 1) % n))
                cur[a], age[a] = q, 1
    return np.stack([np.array(call, np.int32), np.array(dem, np.int32)], -1), took


def sotl_step(scn, tb, st, cur, age, kappa, min_green, theta, mu, **_):
    """One call of SOTL for one instance: cur, age int [A] and kappa int [A, PMAX] are updated in place.  -> (counts int32 [A, PMAX, 2]
    = {call, red(p | cur before the call)}, the branch per agent)."""
    call, _, red = phase_sums(scn, tb, st, cur)
    took = []
    for a in range(scn.n_agent):
        n, c = int(scn.agent_nphase[a]), int(cur[a])
        for p in range(n):
            if p != c:
                kappa[a, p] += red[a][p]
        kappa[a, c] = 0
        if age[a] < min_green:
            age[a] += 1
            took.append(['min_green'])
        elif 0 < call[a][c] <= mu:
            age[a] += 1
            took.append(['platoon'])
        else:
            q = None
            for p in range(n):
                if p != c and (q is None or kappa[a, p] > kappa[a, q]):
                    q = p
            if q is not None and kappa[a, q] >= theta:
                cur[a], age[a], kappa[a, q] = q, 1, 0
                took.append(['change'])
            else:
                age[a] += 1
                took.append(['below'])
        age[a] = min(int(age[a]), 1 << 30)
    return np.stack([np.array(call, np.int32), np.array(red, np.int32)], -1), took


def rule_step(rule, scn, tb, st, state, e, params):
    """gap_step / sotl_step on instance e of state = (cur, age, kappa) [E, ...], in place."""
    cur, age, kappa = state
    if rule == 'actuated':
        return gap_step(scn, tb, st, cur[e], age[e], **params)
    return sotl_step(scn, tb, st, cur[e], age[e], kappa[e], **params)


def count_branches(total, took):
    for names in took:
        for k in names:
            total[k] = total.get(k, 0) + 1


def closed_loop(scn, rule, params, seeds, steps):
    """OracleEnvs of the seeds driven by the loop rule for `steps` control steps -> the branches taken, {name: times}, over all."""
    from oracle.env_oracle import OracleEnv
    tb = tables(scn, rule, params)
    total = {}
    for seed in seeds:
        o = OracleEnv(scn, seed=seed)
        o.reset()
        state = initial_state(scn, 1, params['min_green'])
        for _ in range(steps):
            _, took = rule_step(rule, scn, tb, o.ms.snapshot(), state, 0, params)
            count_branches(total, took)
            o.step(list(state[0][0]))
    return total
