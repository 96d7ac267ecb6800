"""`Interpreter::execute` and `execute_solver`, restated over big integers — TEST INFRASTRUCTURE, the reference of
tests/test_device_exec.py.  It never calls the library.

The statements are `serde_model`'s values (what `serde_model.program_file` encodes), so the program a test executes here and the
bytes it hands to the library come from one description:

  ("Constraint", {"span", "quad": {"span", "left": LinComb, "right": LinComb}, "lin": LinComb, "error"})
  ("Directive",  {"span", "inputs": [QuadComb], "outputs": [{"id": v}], "solver": "Name" | ("Name", payload)})
  ("Log",        {...})
  LinComb = {"span", "value": [({"id": v}, coefficient)]}

Rules restated (reference file:line):
  the walk, define against check      zokrates_interpreter/src/lib.rs:61-137; LinComb::is_assignee zokrates_ast/src/ir/expression.rs:218-222
  evaluate_lin / evaluate_quad        lib.rs:366-378 (sum over the stored terms; a missing variable is the `.unwrap()` panic: ExecPanic)
  the solvers                         lib.rs:249-307; signatures zokrates_ast/src/common/solvers.rs:52-69
  Bits                                to_bits_be cut to the modulus' bit length, zokrates_field/src/lib.rs:204-208; no out-of-range trial
                                      (Interpreter::default())
"""


class ExecPanic(Exception):
    """Where the reference would panic (a read of an undefined variable, a wrong signature) or return Error::Solver."""


# ---------------- constructors of serde_model values ----------------
def lc(terms):
    return {"span": None, "value": [({"id": v}, c) for v, c in terms]}


def quad(left, right):
    return {"span": None, "left": lc(left), "right": lc(right)}


def constraint(left, right, lin):
    return ("Constraint", {"span": None, "quad": quad(left, right), "lin": lc(lin), "error": None})


def directive(inputs, outputs, solver):
    """inputs: [(left terms, right terms)]; outputs: [ids]; solver: "Name" or ("Name", payload)"""
    return ("Directive", {"span": None, "inputs": [quad(l, r) for l, r in inputs], "outputs": [{"id": v} for v in outputs], "solver": solver})


def log(text="x"):
    return ("Log", {"span": None, "format_string": {"parts": [text]}, "expressions": []})


def parameter(vid, private):
    return {"span": None, "id": {"id": vid}, "private": private}


SIGNATURES = {"ConditionEq": (1, 2), "Div": (2, 1), "Xor": (2, 1), "Or": (2, 1), "ShaAndXorAndXorAnd": (3, 1), "ShaCh": (3, 1), "EuclideanDiv": (2, 2)}


# ---------------- the interpreter ----------------
def _lin(w, comb, r):
    acc = 0
    for var, mult in comb["value"]:
        if var["id"] not in w:
            raise ExecPanic("variable %d is not in the witness" % var["id"])
        acc = (acc + w[var["id"]] * mult) % r
    return acc


def _quad(w, q, r):
    return _lin(w, q["left"], r) * _lin(w, q["right"], r) % r


def solve(solver, inputs, r):
    name, payload = (solver, None) if isinstance(solver, str) else solver
    if name == "Bits":
        n_in, n_out = 1, payload
    elif name in SIGNATURES:
        n_in, n_out = SIGNATURES[name]
    else:
        raise ExecPanic("solver %s" % name)
    if len(inputs) != n_in:
        raise ExecPanic("%s takes %d inputs" % (name, n_in))
    if name == "ConditionEq":
        x = inputs[0]
        res = [0, 1] if x == 0 else [1, pow(x, r - 2, r)]
    elif name == "Bits":
        nbits = r.bit_length()
        bits = [(inputs[0] >> (nbits - 1 - i)) & 1 for i in range(nbits)]         # big-endian, MODULUS_BITS of them
        bits = bits[max(len(bits) - payload, 0):]                                  # the least significant `payload`
        res = [0] * (payload - len(bits)) + bits
    elif name == "Xor":
        x, y = inputs
        res = [(x + y - 2 * x * y) % r]
    elif name == "Or":
        x, y = inputs
        res = [(x + y - x * y) % r]
    elif name == "ShaAndXorAndXorAnd":
        a, b, c = inputs
        res = [(b * c - (2 * b * c - b - c) * a) % r]
    elif name == "ShaCh":
        a, b, c = inputs
        res = [(a * (b - c) + c) % r]
    elif name == "Div":
        a, b = inputs
        res = [1 if b == 0 else a * pow(b, r - 2, r) % r]
    else:       # EuclideanDiv
        n, d = inputs
        q = 0 if d == 0 else n // d
        res = [q, n - d * q]
    assert len(res) == n_out
    return res


def execute(r, arguments, statements, inputs):
    """arguments: serde_model Parameter values; inputs: one integer per argument.  Returns (witness {id: value}, None), or
    (None, k) where statement k of the statements section (logs and directives counted) is the first unsatisfied constraint."""
    if len(arguments) != len(inputs):
        raise ExecPanic("WrongInputCount")
    w = {0: 1}
    for arg, value in zip(arguments, inputs):
        w[arg["id"]["id"]] = value % r
    for k, s in enumerate(statements):
        if isinstance(s, str) or s[0] == "Log":
            continue
        kind, body = s
        if kind == "Constraint":
            value = body["lin"]["value"]
            if len(value) == 1 and value[0][1] == 1 and value[0][0]["id"] not in w:
                w[value[0][0]["id"]] = _quad(w, body["quad"], r)
            elif _quad(w, body["quad"], r) != _lin(w, body["lin"], r):
                return None, k
        else:
            res = solve(body["solver"], [_quad(w, q, r) for q in body["inputs"]], r)
            if len(res) != len(body["outputs"]):
                raise ExecPanic("output count")
            for o, v in zip(body["outputs"], res):
                w[o["id"]] = v
    return w, None


def ir_prog(curve, arguments, statements, return_count):
    """The same program as an oracle.ir.Prog (its constraints; everything else opaque), for ir.ark_order / public_inputs_values."""
    from oracle import ir
    terms = lambda comb: [(v["id"], c) for v, c in comb["value"]]
    stmts = []
    for s in statements:
        if not isinstance(s, str) and s[0] == "Constraint":
            b = s[1]
            stmts.append(ir.Constraint(terms(b["quad"]["left"]), terms(b["quad"]["right"]), terms(b["lin"])))
        else:
            stmts.append(ir.Other("Log", None))
    return ir.Prog(curve, [ir.Parameter(a["id"]["id"], a["private"]) for a in arguments], stmts, return_count=return_count)
