"""Count the lines of Python files that hold code: not blank, not comment-only, not part of a docstring.
    python scripts/count_code_lines.py graphs4cfd_amd/nn/model.py graphs4cfd_amd/nn/rollout.py"""
import ast
import io
import sys
import tokenize

SKIP = (tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENDMARKER)


def code_lines(path: str) -> int:
    src = open(path).read()
    doc, code = set(), set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and ast.get_docstring(node, clean=False) is not None:
            doc.update(range(node.body[0].lineno, node.body[0].end_lineno + 1))
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type not in SKIP:
            code.update(range(tok.start[0], tok.end[0] + 1))
    return len(code - doc)


if __name__ == "__main__":
    counts = [(path, code_lines(path)) for path in sys.argv[1:]]
    for path, n in counts:
        print(f"{n:6d}  {path}")
    print(f"{sum(n for _, n in counts):6d}  total")
