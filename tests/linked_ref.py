"""The rule of LINKED.md in plain Python, over an ngsLD TSV: which rows are linked rows.

Every value is read with float() from the row's own text -- the value "as printed" is by construction what a reader of the table
gets.  The maf comes from the --extend_out columns (maf1, maf2); a table without them needs `maf`, the printed maf of every
label.  The output is the selected lines, unchanged and in the table's order."""
import math

# TSV column (1-based, as --linked_field counts) -> its place after the two labels and dist
FIELDS = {4: 1, 5: 2, 6: 3, 7: 4}


def linked_mask(text: str, field: int = 7, min_weight: float = 0.5, abs_value: bool = True, max_kb_dist: float = math.inf,
                min_maf: float = 0.0, label_cols: int = 1, maf: dict | None = None) -> list[bool]:
    """One entry per row of `text` (a header line "site1\t..." and empty lines are not rows): is it a linked row.  label_cols:
    the TAB-separated columns a label takes (a positions file with an extra column prints it inside both labels).  maf:
    {label: float}, for a table without the extended columns."""
    if field not in FIELDS:
        raise ValueError("field must be a TSV column 4..7")
    base = 2 * label_cols  # (the dist column)
    out = []
    for ln in text.splitlines():
        if not ln or ln.startswith("site1\t"):
            continue
        f = ln.split("\t")
        out.append(False)
        x = float(f[base + FIELDS[field]])
        if not math.isfinite(x):
            continue
        v = abs(x) if abs_value else x
        if not v >= min_weight:
            continue
        if len(f) > base + 5:
            maf1, maf2 = float(f[base + 6]), float(f[base + 7])
        else:
            if maf is None:
                raise ValueError("a table without the extended columns needs the sites' maf")
            maf1, maf2 = maf["\t".join(f[:label_cols])], maf["\t".join(f[label_cols:base])]
        if not (maf1 >= min_maf and maf2 >= min_maf):  # (a NaN maf never passes)
            continue
        if math.isfinite(max_kb_dist):  # (the default: no condition on dist at all)
            dist = float(f[base])
            if not (math.isfinite(dist) and dist <= max_kb_dist * 1000):
                continue
        out[-1] = True
    return out


def linked_lines(text: str, **kw) -> list[str]:
    """The linked rows of `text`, unchanged and in its order."""
    rows = [ln for ln in text.splitlines() if ln and not ln.startswith("site1\t")]
    return [ln for ln, m in zip(rows, linked_mask(text, **kw)) if m]


def linked(text: str, header: bool = False, **kw) -> str:
    """The file --linked_out (header False) or --linked_outH (True) writes for this table."""
    head = ""
    if header:
        first = text.split("\n", 1)[0]
        assert first.startswith("site1\t")
        head = first + "\n"
    return head + "".join(ln + "\n" for ln in linked_lines(text, **kw))
