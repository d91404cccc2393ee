#!/usr/bin/env python3
"""What the trainer and scripts/train.py must agree with the reference on, as data: tests/golden/trainer_kat.json.

  config_fields    TrainingConfig's fields (src/training/trainer.py), in order: [name, annotation, default]
  train_flags      scripts/train.py's flags, in order: {name, type, default, choices, action}
  checkpoint_keys  the keys save_checkpoint always writes;  checkpoint_optional_keys  those it adds when EMA / a scaler exist

The two files are parsed, not imported (the trainer needs torchvision and tqdm, which are not installed): the values are the
literals of the class body, of the add_argument calls and of the checkpoint dictionary.  Runs only where the reference exists.
"""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as G  # noqa: E402  (where the reference lies)


def parse(path):
    with open(path, encoding="utf-8") as f:
        return ast.parse(f.read())


def config_fields(tree):
    cls = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == "TrainingConfig")
    return [[n.target.id, ast.unparse(n.annotation), ast.literal_eval(n.value)] for n in cls.body if isinstance(n, ast.AnnAssign)]


def checkpoint_keys(tree):
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "save_checkpoint")
    always, optional = [], []
    for n in ast.walk(fn):
        if isinstance(n, ast.Assign) and isinstance(n.value, ast.Dict) and getattr(n.targets[0], "id", None) == "checkpoint":
            always = [ast.literal_eval(k) for k in n.value.keys]
        elif isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Subscript) and getattr(n.targets[0].value, "id", None) == "checkpoint":
            optional.append(ast.literal_eval(n.targets[0].slice))
    return always, optional


def train_flags(tree):
    flags = []
    for n in ast.walk(tree):
        if isinstance(n, ast.Call) and getattr(n.func, "attr", None) == "add_argument":
            kw = {k.arg: k.value for k in n.keywords}
            flags.append({"name": ast.literal_eval(n.args[0]),
                          "type": kw["type"].id if "type" in kw else None,
                          "default": ast.literal_eval(kw["default"]) if "default" in kw else None,
                          "choices": ast.literal_eval(kw["choices"]) if "choices" in kw else None,
                          "action": ast.literal_eval(kw["action"]) if "action" in kw else None,
                          "line": n.lineno})
    flags.sort(key=lambda f: f.pop("line"))
    return flags


def main():
    trainer = parse(os.path.join(G.REF, "src/training/trainer.py"))
    always, optional = checkpoint_keys(trainer)
    kat = {"config_fields": config_fields(trainer), "train_flags": train_flags(parse(os.path.join(G.REF, "scripts/train.py"))),
           "checkpoint_keys": always, "checkpoint_optional_keys": optional}
    out = os.path.join(ROOT, "tests", "golden", "trainer_kat.json")
    with open(out, "w") as f:
        json.dump(kat, f, indent=1)
        f.write("\n")
    print(f"{out}: {len(kat['config_fields'])} config fields, {len(kat['train_flags'])} flags, keys {always} + {optional}")


if __name__ == "__main__":
    main()
