"""The command-line options of the avatar stages as data: names and settings of every argparse action, without help texts.

    python tests/tools/cli_options.py [--out tests/golden/cli_options.json]

Each stage's parser is captured by intercepting ArgumentParser.parse_args while the module's main() runs, so the tool does not
depend on how a module builds its parser.  For every action: option strings, dest, default, nargs, choices, required, the names
of its action class and type, and the members of its mutually exclusive group (None outside one).  tests/test_avatar_cpu.py holds
the working tree against tests/golden/cli_options.json, which this tool wrote before the stages' front ends were merged."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# command -> (module, the argv that reaches its parser)
COMMANDS = {"skinning": ("skinning", []), "surface": ("surface", []), "render": ("render", []), "decoder": ("decoder", []),
            "texture": ("texture", []), "encoder": ("encoder", []), "scene": ("scene", []), "video": ("video", []),
            "video --extract": ("video", ["--extract", "clip.avi"])}


class _Captured(Exception):
    pass


def captured_parser(module: str, argv) -> argparse.ArgumentParser:
    """The ArgumentParser on which audio2photoreal_amd.<module>.main(argv) calls parse_args."""
    main = importlib.import_module(f"audio2photoreal_amd.{module}").main
    original = argparse.ArgumentParser.parse_args

    def intercept(self, *args, **kw):
        raise _Captured(self)

    argparse.ArgumentParser.parse_args = intercept
    try:
        main(list(argv))
    except _Captured as caught:
        return caught.args[0]
    finally:
        argparse.ArgumentParser.parse_args = original
    raise RuntimeError(f"audio2photoreal_amd.{module}.main({argv}) returned without parsing arguments")


def describe(ap: argparse.ArgumentParser) -> dict:
    groups = {}
    for g in ap._mutually_exclusive_groups:
        members = sorted(a.dest for a in g._group_actions)
        for a in g._group_actions:
            groups[a.dest] = {"members": members, "required": bool(g.required)}
    actions = []
    for a in ap._actions:
        if isinstance(a, argparse._HelpAction):
            continue
        actions.append({"option_strings": list(a.option_strings), "dest": a.dest, "default": a.default, "nargs": a.nargs,
                        "choices": None if a.choices is None else list(a.choices), "required": bool(a.required),
                        "action": type(a).__name__, "type": None if a.type is None else a.type.__name__,
                        "exclusive_group": groups.get(a.dest)})
    return {"prog": ap.prog, "actions": sorted(actions, key=lambda d: d["dest"])}


def cli_options() -> dict:
    """{command: description}, as JSON gives it back (tuples as lists)."""
    return json.loads(json.dumps({name: describe(captured_parser(module, argv)) for name, (module, argv) in COMMANDS.items()}))


if __name__ == "__main__":
    cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    cli.add_argument("--out", default=None, help="write the JSON here (default: print it)")
    out = cli.parse_args().out
    text = json.dumps(cli_options(), indent=1, sort_keys=True) + "\n"
    if out is None:
        sys.stdout.write(text)
    else:
        with open(out, "w") as f:
            f.write(text)
