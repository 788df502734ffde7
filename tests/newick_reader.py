"""A small reader of Newick lines for the tests of the rooted trees (tests/test_root_*.py): the text as nested nodes, the leaf
set below a node, and the splits of a tree with what stands on their branches."""


def parse(text):
    """a Newick line as nested nodes: {"kids": [...], "name", "label", "len" (the text behind the colon)}"""
    assert text.endswith(";\n")
    pos, stack, root = 0, [], None
    text = text[:-2]

    def token(stops):
        nonlocal pos
        if pos < len(text) and text[pos] == "'":
            out, pos = "", pos + 1
            while True:
                if text[pos] == "'" and text[pos + 1:pos + 2] == "'":
                    out, pos = out + "'", pos + 2
                elif text[pos] == "'":
                    pos += 1
                    return out
                else:
                    out, pos = out + text[pos], pos + 1
        start = pos
        while pos < len(text) and text[pos] not in stops:
            pos += 1
        return text[start:pos]

    while pos < len(text):
        ch = text[pos]
        if ch == "(":
            node = {"kids": [], "name": None, "label": "", "len": None}
            if stack:
                stack[-1]["kids"].append(node)
            else:
                root = node
            stack.append(node)
            pos += 1
        elif ch == ",":
            pos += 1
        elif ch == ")":
            pos += 1
            node = stack.pop()
            node["label"] = token(":,()")
            if pos < len(text) and text[pos] == ":":
                pos += 1
                node["len"] = token(",()")
        else:
            node = {"kids": [], "name": token(":"), "label": "", "len": None}
            assert text[pos] == ":"
            pos += 1
            node["len"] = token(",()")
            stack[-1]["kids"].append(node)
    assert not stack
    return root


def leafset(node, index):
    if not node["kids"]:
        return frozenset([index[node["name"]]])
    return frozenset().union(*[leafset(k, index) for k in node["kids"]])


def splits(node, index, n, out, root=True):
    """{canonical side: [(length text, label), ...]} of every node below the root"""
    for k in node["kids"]:
        s = leafset(k, index)
        side = s if 0 not in s else frozenset(range(n)) - s
        out.setdefault(side, []).append((k["len"], k["label"]))
        splits(k, index, n, out, False)
    return out
