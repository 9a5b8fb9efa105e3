"""A PromQL subset: instant-vector selectors and simple aggregations.

Enough for every query the reference issues (``app.py:157`` node discovery:
``kube_pod_info{pod=~".*<pod>.*"}``; ``app.py:167-172`` metric fetch:
``{__name__=~"a|b|c", instance=~"<ip>:.+"}``) plus what the new panels and the
K8s deployment's recording rules use:

    selector   := [metric_name] ['{' matcher (',' matcher)* [','] '}']
    matcher    := label ('=' | '!=' | '=~' | '!~') string
    aggregate  := ('sum'|'avg'|'min'|'max'|'count') [('by'|'without') '(' labels ')']
                  '(' selector ')' [('by'|'without') '(' labels ')']
    quantile   := 'histogram_quantile' '(' number ',' (selector | aggregate) ')'

``histogram_quantile`` has Prometheus' semantics over cumulative ``le`` buckets (here the
window distributions, ``rocmdash_window_bucket``): see :func:`bucket_quantile`.

Regex matchers are fully anchored, as in Prometheus. A selector must contain at
least one matcher that does not match the empty string (Prometheus' rule).
"""

from __future__ import annotations

import math
import re
from dataclasses import dataclass, field

_IDENT = re.compile(r"[a-zA-Z_:][a-zA-Z0-9_:]*")
_LABEL = re.compile(r"[a-zA-Z_][a-zA-Z0-9_]*")
_AGGS = ("sum", "avg", "min", "max", "count")


class PromQLError(ValueError):
    pass


@dataclass(frozen=True)
class Matcher:
    label: str
    op: str
    value: str
    _re: object = field(default=None, compare=False, repr=False)

    @staticmethod
    def make(label: str, op: str, value: str) -> "Matcher":
        rx = None
        if op in ("=~", "!~"):
            try:
                rx = re.compile(f"(?:{value})\\Z", re.DOTALL)
            except re.error as exc:
                raise PromQLError(f"invalid regex {value!r}: {exc}") from exc
        return Matcher(label, op, value, rx)

    def matches(self, v: str) -> bool:
        if self.op == "=":
            return v == self.value
        if self.op == "!=":
            return v != self.value
        hit = self._re.match(v) is not None
        return hit if self.op == "=~" else not hit


@dataclass(frozen=True)
class Selector:
    matchers: tuple

    def matches(self, labels: dict) -> bool:
        for m in self.matchers:
            if not m.matches(labels.get(m.label, "")):
                return False
        return True

    @property
    def metric_name(self):
        for m in self.matchers:
            if m.label == "__name__" and m.op == "=":
                return m.value
        return None


@dataclass(frozen=True)
class Aggregate:
    op: str
    selector: Selector
    by: tuple | None = None
    without: tuple | None = None


@dataclass(frozen=True)
class HistogramQuantile:
    phi: float
    inner: object  # Selector or Aggregate: the bucket series


class _Lexer:
    def __init__(self, s: str):
        self.s = s
        self.i = 0

    def ws(self):
        while self.i < len(self.s) and self.s[self.i].isspace():
            self.i += 1

    def peek(self, tok: str) -> bool:
        self.ws()
        return self.s.startswith(tok, self.i)

    def eat(self, tok: str) -> bool:
        if self.peek(tok):
            self.i += len(tok)
            return True
        return False

    def expect(self, tok: str):
        if not self.eat(tok):
            raise PromQLError(f"expected {tok!r} at position {self.i} in {self.s!r}")

    def ident(self, rx=_IDENT):
        self.ws()
        m = rx.match(self.s, self.i)
        if not m:
            return None
        self.i = m.end()
        return m.group(0)

    def string(self) -> str:
        self.ws()
        if self.i >= len(self.s) or self.s[self.i] not in "\"'`":
            raise PromQLError(f"expected a string at position {self.i} in {self.s!r}")
        q = self.s[self.i]
        self.i += 1
        out = []
        while self.i < len(self.s):
            c = self.s[self.i]
            if c == q:
                self.i += 1
                return "".join(out)
            if c == "\\" and q != "`" and self.i + 1 < len(self.s):
                n = self.s[self.i + 1]
                out.append({"n": "\n", "t": "\t", "\\": "\\", '"': '"', "'": "'"}.get(n, "\\" + n))
                self.i += 2
                continue
            out.append(c)
            self.i += 1
        raise PromQLError("unterminated string")

    def done(self) -> bool:
        self.ws()
        return self.i >= len(self.s)


def _parse_selector(lx: _Lexer) -> Selector:
    name = lx.ident()
    matchers = []
    if name is not None:
        if name in _AGGS or name in ("by", "without"):
            raise PromQLError(f"unexpected keyword {name!r}")
        matchers.append(Matcher.make("__name__", "=", name))
    if lx.eat("{"):
        while not lx.eat("}"):
            label = lx.ident(_LABEL)
            if label is None:
                raise PromQLError(f"expected a label name at position {lx.i}")
            for op in ("=~", "!~", "!=", "="):
                if lx.eat(op):
                    break
            else:
                raise PromQLError(f"expected a matcher operator at position {lx.i}")
            matchers.append(Matcher.make(label, op, lx.string()))
            if not lx.eat(","):
                lx.expect("}")
                break
    if not matchers:
        raise PromQLError("empty selector")
    if all(m.matches("") for m in matchers):
        raise PromQLError("vector selector must contain at least one non-empty matcher")
    return Selector(tuple(matchers))


def _parse_grouping(lx: _Lexer):
    for kw in ("by", "without"):
        save = lx.i
        if lx.ident() == kw:
            lx.expect("(")
            labels = []
            while not lx.eat(")"):
                lab = lx.ident(_LABEL)
                if lab is None:
                    raise PromQLError("expected a label in grouping")
                labels.append(lab)
                if not lx.eat(","):
                    lx.expect(")")
                    break
            return kw, tuple(labels)
        lx.i = save
    return None, None


_NUMBER = re.compile(r"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[+-]?(?:[iI]nf|NaN)")


def _parse_vector(lx: _Lexer):
    """A ``Selector`` or an ``Aggregate`` at the lexer's position."""
    save = lx.i
    word = lx.ident()
    if word in _AGGS:
        kw, labels = _parse_grouping(lx)
        lx.expect("(")
        sel = _parse_selector(lx)
        lx.expect(")")
        if kw is None:
            kw, labels = _parse_grouping(lx)
        return Aggregate(word, sel, labels if kw == "by" else None, labels if kw == "without" else None)
    lx.i = save
    return _parse_selector(lx)


def parse(query: str):
    """Parse a query into a ``Selector``, an ``Aggregate`` or a ``HistogramQuantile``."""
    lx = _Lexer(query.strip())
    save = lx.i
    if lx.ident() == "histogram_quantile" and lx.eat("("):
        num = lx.ident(_NUMBER)
        if num is None:
            raise PromQLError(f"expected the quantile (a number) at position {lx.i}")
        lx.expect(",")
        expr = HistogramQuantile(float(num), _parse_vector(lx))
        lx.expect(")")
    else:
        lx.i = save
        expr = _parse_vector(lx)
    if not lx.done():
        raise PromQLError(f"unexpected trailing input at position {lx.i}")
    return expr


def aggregate(expr: Aggregate, series: list) -> list:
    """``series``: [(labels_dict, value)] matched by the selector -> aggregated list."""
    groups: dict = {}
    for labels, v in series:
        if expr.by is not None:
            key = tuple((k, labels[k]) for k in expr.by if k in labels)
        elif expr.without is None:  # plain `sum(x)`: one group, no labels
            key = ()
        else:
            drop = set(expr.without or ()) | {"__name__"}
            key = tuple(sorted((k, x) for k, x in labels.items() if k not in drop))
        groups.setdefault(key, []).append(v)
    out = []
    for key, vals in groups.items():
        finite = [x for x in vals if not math.isnan(x)]
        if expr.op == "count":
            r = float(len(vals))
        elif expr.op == "sum":
            r = float(sum(vals))
        elif expr.op == "avg":
            r = float(sum(vals)) / len(vals)
        elif expr.op == "min":
            r = min(finite) if finite else float("nan")
        else:
            r = max(finite) if finite else float("nan")
        out.append((dict(key), r))
    return out


def bucket_quantile(phi: float, buckets: list) -> float:
    """Prometheus' ``histogram_quantile`` of one histogram: ``buckets`` [(le, cumulative
    count)]. Buckets are sorted by ``le`` (equal bounds merged, counts made monotone); the
    quantile is interpolated linearly inside its bucket, whose lower edge is the previous
    bound - 0 for the first bucket when its bound is > 0 (a first bound <= 0 is returned as
    it is). A quantile in the ``+Inf`` bucket gives the highest finite bound. NaN without a
    ``+Inf`` bucket, without a finite one or without samples; -Inf / +Inf for phi < 0 / > 1."""
    if math.isnan(phi):
        return float("nan")
    if phi < 0:
        return float("-inf")
    if phi > 1:
        return float("inf")
    bs = sorted((float(le), float(c)) for le, c in buckets if not math.isnan(float(le)))
    if not bs or bs[-1][0] != float("inf"):
        return float("nan")
    merged = []
    for le, c in bs:
        if merged and merged[-1][0] == le:
            merged[-1][1] += c
        else:
            merged.append([le, c])
    for i in range(1, len(merged)):  # cumulative counts never go down
        merged[i][1] = max(merged[i][1], merged[i - 1][1])
    if len(merged) < 2:
        return float("nan")
    total = merged[-1][1]
    if not total > 0:
        return float("nan")
    rank = phi * total
    b = next((i for i in range(len(merged) - 1) if merged[i][1] >= rank), len(merged) - 1)
    if b == len(merged) - 1:
        return merged[-2][0]
    if b == 0 and merged[0][0] <= 0:
        return merged[0][0]
    start, end, count = 0.0, merged[b][0], merged[b][1]
    if b > 0:
        start = merged[b - 1][0]
        count -= merged[b - 1][1]
        rank -= merged[b - 1][1]
    return start + (end - start) * (rank / count)


def histogram_quantile(phi: float, series: list) -> list:
    """``series``: [(labels_dict, value)] of bucket series -> [(labels, quantile)], one per
    group of all labels but ``le`` (and the metric name). Series without a parsable ``le``
    are ignored, as Prometheus does."""
    groups: dict = {}
    for labels, v in series:
        try:
            le = float(labels["le"])
        except (KeyError, ValueError):
            continue
        key = tuple(sorted((k, x) for k, x in labels.items() if k not in ("le", "__name__")))
        groups.setdefault(key, []).append((le, v))
    return [(dict(key), bucket_quantile(phi, b)) for key, b in groups.items()]
